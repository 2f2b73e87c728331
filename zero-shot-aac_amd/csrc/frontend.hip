// Audio front end: fused STFT power -> Slaney mel -> 10*log10 -> bn0 (torchlibrosa Spectrogram +
// LogmelFilterBank, retrieval/models/feature_extractor.py:16-38; bn0 htsat.py:949-951), the
// HTSAT bicubic resize + fold (htsat.py:908-923) and PatchEmbed + LayerNorm (htsat.py:115-125).
//
// STFT: one 256-thread block per LM_PAIRS pairs of frames: two real, reflect-padded,
// Hann-windowed 1024-sample frames are packed as z = a + i*b, loaded (coalesced) into padded LDS
// rows in natural order and transformed with a radix-4 decimation-in-frequency complex FFT (5
// stages, one radix-4 butterfly per thread per pair per stage, twiddles from a host table staged
// in LDS; the output lands in base-4 digit-reversed order); the two spectra are
// separated as A_k = (Z_k + conj Z_{N-k})/2, B_k = (Z_k - conj Z_{N-k})/2i, |.|^2 for k <= 512,
// then 64 threads per frame contract the power spectrum with their mel filter's nonzero band.
#include "common.h"

namespace zs {

constexpr int NFFT = 1024, HOP = 320, NMEL = 64, NBIN = NFFT / 2 + 1;

__device__ __forceinline__ int digrev4(int n) {   // reverse the 5 base-4 digits of n < 1024
  int r = 0;
#pragma unroll
  for (int d = 0; d < 5; ++d) { r = (r << 2) | (n & 3); n >>= 2; }
  return r;
}

constexpr int LM_PAIRS = 2;               // frame pairs (complex FFTs) per 256-thread block
constexpr int LPAD = NFFT + NFFT / 16;     // padded LDS row: element i lives at i + i/16
__device__ __forceinline__ int lp(int i) { return i + (i >> 4); }

__global__ __launch_bounds__(256) void logmel_kernel(
    const float* __restrict__ wav, int T, int n_frames, int total_frames,
    const float* __restrict__ window, const float* __restrict__ twiddle,
    const float* __restrict__ melW, const int* __restrict__ mel_lo, const int* __restrict__ mel_hi,
    const float* __restrict__ bn_mean, const float* __restrict__ bn_var,
    const float* __restrict__ bn_w, const float* __restrict__ bn_b, float* __restrict__ out) {
  constexpr int NP = LM_PAIRS;
  __shared__ float re[NP][LPAD], im[NP][LPAD];
  __shared__ float tw[NFFT];              // (cos, sin)(-2 pi k / 1024), k < 512
  __shared__ float mw[2 * NBIN];          // the mel filters' nonzero bands, packed
  __shared__ float pw[2 * NP][NBIN];
  __shared__ int moff[NMEL + 1], mlo[NMEL];
  for (int n = threadIdx.x; n < NFFT; n += 256) tw[n] = twiddle[n];
  if (threadIdx.x < 64) {                 // band offsets: wave-wide inclusive scan of the widths
    const int m = threadIdx.x;
    const int lo = mel_lo[m], len = mel_hi[m] - lo;
    int inc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (m >= d) inc += o;
    }
    mlo[m] = lo;
    moff[m + 1] = inc;
    if (m == 0) moff[0] = 0;
  }
  __syncthreads();
  {   // pack the bands: 4 threads per mel filter
    const int m = threadIdx.x >> 2, s0 = threadIdx.x & 3;
    const int lo = mlo[m], len = moff[m + 1] - moff[m];
    for (int k = s0; k < len; k += 4) mw[moff[m] + k] = melW[m * NBIN + lo + k];
  }
  // persistent over frame groups: the twiddles and the packed mel bands are staged once per block
  for (int g0 = 2 * NP * blockIdx.x; g0 < total_frames; g0 += 2 * NP * gridDim.x) {
  // natural-order load (coalesced global reads, conflict-free LDS writes)
  for (int n = threadIdx.x; n < NP * NFFT; n += 256) {
    const int p = n / NFFT, k = n % NFFT;
    float v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int g = g0 + 2 * p + q;
      v[q] = 0.f;
      if (g < total_frames) {
        const int b = g / n_frames, f = g % n_frames;
        int o = f * HOP - NFFT / 2 + k;
        if (o < 0) o = -o;                       // reflect (no edge repeat), torch F.pad 'reflect'
        if (o >= T) o = 2 * (T - 1) - o;
        v[q] = wav[(long)b * T + o] * window[k];
      }
    }
    re[p][lp(k)] = v[0];
    im[p][lp(k)] = v[1];
  }
  __syncthreads();
  // radix-4 DIF (natural-order in, base-4 digit-reversed out):
  // y0 = x0+x1+x2+x3, y1 = (x0-x2) - i(x1-x3), y2 = (x0+x2) - (x1+x3), y3 = (x0-x2) + i(x1-x3),
  // then y_p *= W_{4L}^{p j} = W_1024^{p j S}
  for (int L = NFFT / 4, S = 1; L >= 1; L >>= 2, S <<= 2) {
    const int bf = threadIdx.x, grp = bf / L, j = bf % L;
    const int i0 = grp * 4 * L + j;
    float wr[4], wi[4];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const int e = j * q * S;                   // < 768
      if (e < 512) { wr[q] = tw[2 * e]; wi[q] = tw[2 * e + 1]; }
      else { wr[q] = -tw[2 * (e - 512)]; wi[q] = -tw[2 * (e - 512) + 1]; }
    }
    float xr[NP][4], xi[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) { xr[p][q] = re[p][lp(i0 + q * L)]; xi[p][q] = im[p][lp(i0 + q * L)]; }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float s02r = xr[p][0] + xr[p][2], s02i = xi[p][0] + xi[p][2];
      const float d02r = xr[p][0] - xr[p][2], d02i = xi[p][0] - xi[p][2];
      const float s13r = xr[p][1] + xr[p][3], s13i = xi[p][1] + xi[p][3];
      const float d13r = xr[p][1] - xr[p][3], d13i = xi[p][1] - xi[p][3];
      float yr[4], yi[4];
      yr[0] = s02r + s13r; yi[0] = s02i + s13i;
      yr[1] = d02r + d13i; yi[1] = d02i - d13r;
      yr[2] = s02r - s13r; yi[2] = s02i - s13i;
      yr[3] = d02r - d13i; yi[3] = d02i + d13r;
      re[p][lp(i0)] = yr[0];
      im[p][lp(i0)] = yi[0];
#pragma unroll
      for (int q = 1; q < 4; ++q) {
        re[p][lp(i0 + q * L)] = yr[q] * wr[q] - yi[q] * wi[q];
        im[p][lp(i0 + q * L)] = yr[q] * wi[q] + yi[q] * wr[q];
      }
    }
    __syncthreads();
  }
  // X[k] sits at digrev4(k); separate the two real spectra, |.|^2 for k <= 512
  for (int n = threadIdx.x; n < NP * NBIN; n += 256) {
    const int p = n / NBIN, k = n % NBIN;
    const int a = lp(digrev4(k)), c = lp(digrev4((NFFT - k) & (NFFT - 1)));
    const float zr = re[p][a], zi = im[p][a], cr = re[p][c], ci = -im[p][c];   // conj Z_{N-k}
    const float ar = zr + cr, ai = zi + ci;        // 2 A_k
    const float br = zi - ci, bi = cr - zr;        // 2 B_k = (Z - conj Z_{N-k}) / i
    pw[2 * p][k] = 0.25f * (ar * ar + ai * ai);
    pw[2 * p + 1][k] = 0.25f * (br * br + bi * bi);
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 2 * NP * NMEL; o += 256) {
    const int fr = o / NMEL, m = o % NMEL;
    const int g = g0 + fr;
    if (g >= total_frames) continue;
    const int lo = mlo[m], base = moff[m], len = moff[m + 1] - base;
    float acc = 0.f;
    for (int k = 0; k < len; ++k) acc += pw[fr][lo + k] * mw[base + k];
    float v = 10.0f * log10f(fmaxf(acc, 1e-10f));   // power_to_db, ref 1.0 -> offset 0
    if (bn_mean) v = (v - bn_mean[m]) / sqrtf(bn_var[m] + 1e-5f) * bn_w[m] + bn_b[m];
    out[(long)g * NMEL + m] = v;
  }
  __syncthreads();   // re/im/pw are refilled by the next group
  }
}

// ------------------------------------------------------------------ wave-per-FFT front end
// One wave per frame pair (complex 1024-point FFT), 4 independent waves per block, no block
// barriers in the frame loop.  The same radix-4 DIF as logmel_kernel (same twiddles, same
// butterfly arithmetic), but with the 16 points a lane holds two stages run in registers between
// LDS exchanges (3 exchanges instead of 5 block-wide stage round trips):
//   phase 1: lane l holds n = 256a + 64b + l            -> stages over a, b
//   phase 2: lane (p1, p2, e) holds 256p1+64p2+16c+4d+e -> stages over c, d
//   phase 3: lane l holds 16l + 4r + e (r = 0..3)        -> the last stage over e
// Every exchange is conflict-free in the padded row (i + i/16).  The wave's row then holds the
// spectrum in base-4 digit-reversed order; the two real spectra are separated into power rows
// (aliasing the row: each lane's reads finish before its writes, LDS ops of a wave are in
// order) and lane m contracts mel band m for both frames.
__device__ __forceinline__ float2 twd(const float* tw, int e) {   // W_1024^e, e < 1024
  if (e < 512) return make_float2(tw[2 * e], tw[2 * e + 1]);
  return make_float2(-tw[2 * (e - 512)], -tw[2 * (e - 512) + 1]);
}
__device__ __forceinline__ void bfly4(float (&xr)[4], float (&xi)[4]) {
  const float s02r = xr[0] + xr[2], s02i = xi[0] + xi[2];
  const float d02r = xr[0] - xr[2], d02i = xi[0] - xi[2];
  const float s13r = xr[1] + xr[3], s13i = xi[1] + xi[3];
  const float d13r = xr[1] - xr[3], d13i = xi[1] - xi[3];
  xr[0] = s02r + s13r; xi[0] = s02i + s13i;
  xr[1] = d02r + d13i; xi[1] = d02i - d13r;
  xr[2] = s02r - s13r; xi[2] = s02i - s13i;
  xr[3] = d02r - d13i; xi[3] = d02i + d13r;
}
__device__ __forceinline__ void twmul(float& r, float& i, float2 w) {
  const float t = r * w.x - i * w.y;
  i = r * w.y + i * w.x;
  r = t;
}
// W_1024^{64 m} = W_16^m (m < 16): exact-rounded constants, folded after unrolling
__device__ __forceinline__ float2 w16(int m) {
  constexpr float C[16] = {1.f, 0.92387953f, 0.70710678f, 0.38268343f, 0.f, -0.38268343f,
                           -0.70710678f, -0.92387953f, -1.f, -0.92387953f, -0.70710678f,
                           -0.38268343f, 0.f, 0.38268343f, 0.70710678f, 0.92387953f};
  return make_float2(C[m & 15], C[(m + 4) & 15]);   // (cos, -sin)(2 pi m / 16)
}
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// orders this wave's LDS accesses for the compiler (the hardware keeps a wave's LDS ops in order)
__device__ __forceinline__ void wave_lds_order() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

int g_logmel_wave = 1;   // zs_tune_set("logmel_wave", 0): the block-per-4-frames kernel

__global__ __launch_bounds__(256, 3) void logmel_wave_kernel(
    const float* __restrict__ wav, int T, int n_frames, int total_frames,
    const float* __restrict__ window, const float* __restrict__ twiddle,
    const float* __restrict__ melW, const int* __restrict__ mel_lo, const int* __restrict__ mel_hi,
    const float* __restrict__ bn_mean, const float* __restrict__ bn_var,
    const float* __restrict__ bn_w, const float* __restrict__ bn_b, float* __restrict__ out) {
  __shared__ float rows[4][2][LPAD];      // per wave: re, im (later: the two power rows)
  __shared__ float tw[NFFT];
  __shared__ float swin[NFFT];
  __shared__ float mw[2 * NBIN];
  __shared__ int moff[NMEL + 1], mlo[NMEL];
  for (int n = threadIdx.x; n < NFFT; n += 256) { tw[n] = twiddle[n]; swin[n] = window[n]; }
  if (threadIdx.x < 64) {
    const int m = threadIdx.x;
    const int lo = mel_lo[m], len = mel_hi[m] - lo;
    int inc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (m >= d) inc += o;
    }
    mlo[m] = lo;
    moff[m + 1] = inc;
    if (m == 0) moff[0] = 0;
  }
  __syncthreads();
  {
    const int m = threadIdx.x >> 2, s0 = threadIdx.x & 3;
    const int lo = mlo[m], len = moff[m + 1] - moff[m];
    for (int k = s0; k < len; k += 4) mw[moff[m] + k] = melW[m * NBIN + lo + k];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float* re = rows[wid][0];
  float* im = rows[wid][1];
  const int npairs = (total_frames + 1) >> 1;
  // raw samples of a pair (zero for a missing second frame); the next pair's are fetched before
  // the current pair's FFT so their HBM latency overlaps it
  auto fetch = [&](int gp, float (&sr)[16], float (&si)[16]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int g = 2 * gp + q;
      const bool valid = g < total_frames;
      const int gb = valid ? g / n_frames : 0, f = valid ? g % n_frames : 0;
      const float* src = wav + (long)gb * T;
      const int base = f * HOP - NFFT / 2;
      if (valid && base >= 0 && base + NFFT <= T) {   // interior frame (wave-uniform): one
        const float* p = src + base + lane;            // pointer, immediate offsets
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (q == 0) sr[i] = p[64 * i]; else si[i] = p[64 * i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int o = base + 64 * i + lane;
          if (o < 0) o = -o;                       // reflect (no edge repeat), torch F.pad 'reflect'
          if (o >= T) o = 2 * (T - 1) - o;
          const float v = valid ? src[o] : 0.f;
          if (q == 0) sr[i] = v; else si[i] = v;
        }
      }
    }
  };
  const int stride = gridDim.x * 4;
  float cr_[16], ci_[16];
  int gp = blockIdx.x * 4 + wid;
  if (gp < npairs) fetch(gp, cr_, ci_);
  for (; gp < npairs; gp += stride) {
    float zr[4][4], zi[4][4];             // phase 1: [a][b], n = 256a + 64b + lane
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float wv = swin[256 * a + 64 * b + lane];
        zr[a][b] = cr_[4 * a + b] * wv;
        zi[a][b] = ci_[4 * a + b] * wv;
      }
    if (gp + stride < npairs) fetch(gp + stride, cr_, ci_);
    // stage 1 (over a), twiddle W_1024^{p (64b + lane)} = W_1024^{p lane} W_16^{p b} (three
    // table twiddles per lane instead of twelve: they stay in registers across the frame loop)
    const float2 t1[4] = {make_float2(1.f, 0.f), twd(tw, lane), twd(tw, 2 * lane), twd(tw, 3 * lane)};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float xr[4] = {zr[0][b], zr[1][b], zr[2][b], zr[3][b]};
      float xi[4] = {zi[0][b], zi[1][b], zi[2][b], zi[3][b]};
      bfly4(xr, xi);
#pragma unroll
      for (int p = 1; p < 4; ++p) twmul(xr[p], xi[p], b == 0 ? t1[p] : cmul(t1[p], w16(p * b)));
#pragma unroll
      for (int p = 0; p < 4; ++p) { zr[p][b] = xr[p]; zi[p][b] = xi[p]; }
    }
    // stage 2 (over b), twiddle W_1024^{4 p lane}
    {
      const float2 w1 = twd(tw, 4 * lane), w2 = twd(tw, 8 * lane), w3 = twd(tw, 12 * lane);
#pragma unroll
      for (int p1 = 0; p1 < 4; ++p1) {
        float xr[4] = {zr[p1][0], zr[p1][1], zr[p1][2], zr[p1][3]};
        float xi[4] = {zi[p1][0], zi[p1][1], zi[p1][2], zi[p1][3]};
        bfly4(xr, xi);
        twmul(xr[1], xi[1], w1);
        twmul(xr[2], xi[2], w2);
        twmul(xr[3], xi[3], w3);
#pragma unroll
        for (int p = 0; p < 4; ++p) { zr[p1][p] = xr[p]; zi[p1][p] = xi[p]; }
      }
    }
    wave_lds_order();                      // previous pair's mel reads of this row are done
#pragma unroll
    for (int p1 = 0; p1 < 4; ++p1)
#pragma unroll
      for (int p2 = 0; p2 < 4; ++p2) {
        re[lp(256 * p1 + 64 * p2 + lane)] = zr[p1][p2];
        im[lp(256 * p1 + 64 * p2 + lane)] = zi[p1][p2];
      }
    wave_lds_order();
    // phase 2: lane = 16 p1 + 4 p2 + e holds pb + 16c + 4d
    const int E = lane & 3;
    const int pb = 256 * (lane >> 4) + 64 * ((lane >> 2) & 3) + E;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        zr[c][d] = re[lp(pb + 16 * c + 4 * d)];
        zi[c][d] = im[lp(pb + 16 * c + 4 * d)];
      }
    // stage 3 (over c), twiddle W_1024^{16 p (4d + e)} = W_1024^{16 p e} W_16^{p d}
    const float2 t3[4] = {make_float2(1.f, 0.f), twd(tw, 16 * E), twd(tw, 32 * E), twd(tw, 48 * E)};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float xr[4] = {zr[0][d], zr[1][d], zr[2][d], zr[3][d]};
      float xi[4] = {zi[0][d], zi[1][d], zi[2][d], zi[3][d]};
      bfly4(xr, xi);
#pragma unroll
      for (int p = 1; p < 4; ++p) twmul(xr[p], xi[p], d == 0 ? t3[p] : cmul(t3[p], w16(p * d)));
#pragma unroll
      for (int p = 0; p < 4; ++p) { zr[p][d] = xr[p]; zi[p][d] = xi[p]; }
    }
    // stage 4 (over d), twiddle W_1024^{64 p e}
    {
      const float2 w1 = twd(tw, 64 * E), w2 = twd(tw, 128 * E), w3 = twd(tw, 192 * E);
#pragma unroll
      for (int p3 = 0; p3 < 4; ++p3) {
        float xr[4] = {zr[p3][0], zr[p3][1], zr[p3][2], zr[p3][3]};
        float xi[4] = {zi[p3][0], zi[p3][1], zi[p3][2], zi[p3][3]};
        bfly4(xr, xi);
        twmul(xr[1], xi[1], w1);
        twmul(xr[2], xi[2], w2);
        twmul(xr[3], xi[3], w3);
#pragma unroll
        for (int p = 0; p < 4; ++p) { zr[p3][p] = xr[p]; zi[p3][p] = xi[p]; }
      }
    }
    wave_lds_order();
#pragma unroll
    for (int p3 = 0; p3 < 4; ++p3)
#pragma unroll
      for (int p4 = 0; p4 < 4; ++p4) {
        re[lp(pb + 16 * p3 + 4 * p4)] = zr[p3][p4];
        im[lp(pb + 16 * p3 + 4 * p4)] = zi[p3][p4];
      }
    wave_lds_order();
    // phase 3: lane holds 16 lane + 4r + e; the last stage (twiddle 1), written back in place
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float xr[4], xi[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { xr[e] = re[lp(16 * lane + 4 * r + e)]; xi[e] = im[lp(16 * lane + 4 * r + e)]; }
      bfly4(xr, xi);
#pragma unroll
      for (int e = 0; e < 4; ++e) { re[lp(16 * lane + 4 * r + e)] = xr[e]; im[lp(16 * lane + 4 * r + e)] = xi[e]; }
    }
    wave_lds_order();
    // X[k] sits at digrev4(k): separate the two real spectra, |.|^2 for k <= 512
    float pa[9], pq[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int k = min(lane + 64 * t, NBIN - 1);
      const int a = lp(digrev4(k)), c = lp(digrev4((NFFT - k) & (NFFT - 1)));
      const float zr_ = re[a], zi_ = im[a], cr = re[c], ci = -im[c];
      const float ar = zr_ + cr, ai = zi_ + ci;
      const float br = zi_ - ci, bi = cr - zr_;
      pa[t] = 0.25f * (ar * ar + ai * ai);
      pq[t] = 0.25f * (br * br + bi * bi);
    }
    wave_lds_order();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int k = lane + 64 * t;
      if (k < NBIN) { re[k] = pa[t]; im[k] = pq[t]; }
    }
    wave_lds_order();
    {
      const int m = lane;
      const int lo = mlo[m], base = moff[m], len = moff[m + 1] - base;
      float acc0 = 0.f, acc1 = 0.f;
      for (int k = 0; k < len; ++k) {
        const float wv = mw[base + k];
        acc0 += re[lo + k] * wv;
        acc1 += im[lo + k] * wv;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int g = 2 * gp + q;
        if (g >= total_frames) continue;
        float v = 10.0f * log10f(fmaxf(q ? acc1 : acc0, 1e-10f));   // power_to_db, ref 1.0
        if (bn_mean) v = (v - bn_mean[m]) / sqrtf(bn_var[m] + 1e-5f) * bn_w[m] + bn_b[m];
        out[(long)g * NMEL + m] = v;
      }
    }
  }
}

// bicubic (A = -0.75, align_corners = True) along time T_in -> 1024, identity along the 64 mels,
// then fold: img[r = chunk*64 + mel][c] = resized[t = chunk*256 + c][mel]
__global__ void wav2img_kernel(const float* __restrict__ in, int T_in, float* __restrict__ img) {
#pragma clang fp contract(off)   // torch rounds scale*t before `- floor` and each weight term
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = e % 256, r = (e / 256) % 256, b = e / 65536;
  const int chunk = r / 64, mel = r % 64;
  const int t = chunk * 256 + c;
  const float scale = (float)(T_in - 1) / (float)(1024 - 1);
  // rounded product (no FMA contraction into `src - i0`): torch's area_pixel_compute_source_index
  const float src = __fmul_rn(scale, (float)t);
  const int i0 = (int)floorf(src);
  const float x1 = src - (float)i0;
  const float A = -0.75f;
  auto cc1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
  auto cc2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
  const float w0 = cc2(x1 + 1.f), w1 = cc1(x1), x2 = 1.f - x1, w2 = cc1(x2), w3 = cc2(x2 + 1.f);
  const float* col = in + (long)b * T_in * 64 + mel;
  auto at = [&](int i) { i = i < 0 ? 0 : (i >= T_in ? T_in - 1 : i); return col[(long)i * 64]; };
  float v = at(i0 - 1) * w0;
  v += at(i0) * w1;
  v += at(i0 + 1) * w2;
  v += at(i0 + 2) * w3;
  img[e] = v;
}

// PatchEmbed: 4 lanes per token (a 4x4 patch -> 96 channels, 24 per lane, LayerNorm reduced over
// the lane quad); 256 threads = 64 tokens = one row of the 64x64 patch grid, weights / bias / LN
// params broadcast from LDS.  Lane g of a quad owns channels 16i + 4g .. 16i + 4g + 3 (i < 6), so
// each 16-byte store instruction writes 64 contiguous bytes per token.  (One thread per token held
// 96 values, ran at one wave per SIMD and stored 64 scattered lines per instruction.)
__global__ __launch_bounds__(256) void patch_embed_kernel(const float* __restrict__ img,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ lnw,
                                                          const float* __restrict__ lnb,
                                                          float* __restrict__ x, long ntok) {
  constexpr int C = 96, CPL = C / 4, WS = 20;   // weight row stride: 16 + 4 pad (16-B aligned)
  // 20-float rows: the quad's 4 lanes read channels 4 apart, whose rows then start 16 banks apart
  // (a 16-float stride put all four on the same banks: 4-way conflicts on every weight read)
  __shared__ __attribute__((aligned(16))) float sw[C * WS];
  __shared__ float sb[C], sg[C], sbeta[C];
  for (int i = threadIdx.x; i < C * 16; i += 256) sw[(i / 16) * WS + (i % 16)] = w[i];
  if (threadIdx.x < C) {
    sb[threadIdx.x] = bias[threadIdx.x];
    sg[threadIdx.x] = lnw[threadIdx.x];
    sbeta[threadIdx.x] = lnb[threadIdx.x];
  }
  __syncthreads();
  const long tok = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int g = threadIdx.x & 3;
  const bool valid = tok < ntok;          // whole quads (ntok is a multiple of 4096)
  const long tk = valid ? tok : 0;
  const int b = (int)(tk / 4096), t = (int)(tk % 4096), ph = t / 64, pwc = t % 64;
  const float* base = img + (long)b * 65536 + (ph * 4) * 256 + pwc * 4;
  float px[16];
#pragma unroll
  for (int ky = 0; ky < 4; ++ky) {
    const float4 r = *reinterpret_cast<const float4*>(base + ky * 256);
    px[ky * 4 + 0] = r.x; px[ky * 4 + 1] = r.y; px[ky * 4 + 2] = r.z; px[ky * 4 + 3] = r.w;
  }
  float v[CPL];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < CPL / 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 16 * i + 4 * g + j;
      float a = sb[c];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 wq = *reinterpret_cast<const float4*>(sw + c * WS + 4 * q4);
        a += wq.x * px[4 * q4];
        a += wq.y * px[4 * q4 + 1];
        a += wq.z * px[4 * q4 + 2];
        a += wq.w * px[4 * q4 + 3];
      }
      v[4 * i + j] = a;
      sum += a;
    }
  sum += __shfl_xor(sum, 1, 64);
  sum += __shfl_xor(sum, 2, 64);
  const float mean = sum / C;
  float var = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) { const float d = v[k] - mean; var += d * d; }
  var += __shfl_xor(var, 1, 64);
  var += __shfl_xor(var, 2, 64);
  const float rstd = rsqrtf(var / C + 1e-5f);
  if (!valid) return;
#pragma unroll
  for (int i = 0; i < CPL / 4; ++i) {
    const int c = 16 * i + 4 * g;
    *reinterpret_cast<float4*>(x + tok * C + c) =
        make_float4((v[4 * i] - mean) * rstd * sg[c] + sbeta[c],
                    (v[4 * i + 1] - mean) * rstd * sg[c + 1] + sbeta[c + 1],
                    (v[4 * i + 2] - mean) * rstd * sg[c + 2] + sbeta[c + 2],
                    (v[4 * i + 3] - mean) * rstd * sg[c + 3] + sbeta[c + 3]);
  }
}

// Ragged clips -> [B][T] fixed-length rows (data_handing/embeddings_generator.py:53-59): clip b
// (length len[b], starting at off[b] of one flat buffer) is cropped to its first T samples or
// zero-padded at the end.  float4 stores; the source is read with scalar loads (clip offsets
// need not be 16-byte aligned).
__global__ __launch_bounds__(256) void pack_clips_kernel(const float* __restrict__ flat,
                                                         const long* __restrict__ off,
                                                         const int* __restrict__ len, int T,
                                                         float* __restrict__ out) {
  const int b = blockIdx.y;
  const long o = off[b];
  const int n = min(len[b], T);
  for (int i = 4 * (blockIdx.x * 256 + threadIdx.x); i < T; i += 4 * 256 * gridDim.x) {
    float4 v;
    v.x = i < n ? flat[o + i] : 0.f;
    v.y = i + 1 < n ? flat[o + i + 1] : 0.f;
    v.z = i + 2 < n ? flat[o + i + 2] : 0.f;
    v.w = i + 3 < n ? flat[o + i + 3] : 0.f;
    *reinterpret_cast<float4*>(out + (long)b * T + i) = v;
  }
}

// ------------------------------------------------------------------ resample + downmix + pack
// librosa.load(path, sr, mono=True) followed by the crop / pad of
// data_handing/embeddings_generator.py:48-59, for clips that arrive as decoded, interleaved
// frames at their files' own rates: to_mono (np.mean over the channels, f32), resampy's
// resample_f with the kaiser_best table (librosa 0.9.2's default res_type), the first T outputs
// kept and the rest of the row zero.
//
// One 256-thread block per RS_TILE consecutive outputs of one clip.  The tile's input span
// (the samples between its first output's left wing and its last output's right wing) is
// downmixed once into LDS; each lane then accumulates four of the tile's outputs in a register,
// reading (win, delta) pairs of the interleaved table from global memory (256 KB, resident in
// L2; which output a lane takes is chosen so that a wave's lanes read neighbouring phases:
// rs_stride).
//
// Time base: output t sits at input time t * sr_in / sr_out.  p = t * sr_in is a 64-bit integer,
// n = p / sr_out the sample left of it and r = p % sr_out the exact remainder, so the table
// phase frac * nb = scale * nb * r / sr_out = nb * r / max(sr_in, sr_out) is an integer quotient
// (the table offset) and an integer remainder (eta's numerator): no rounding until eta itself,
// and no dependence between outputs (resampy adds 1/ratio into a float64 register per output).
constexpr int RS_TILE = 1024;             // outputs per block (4 per lane)
constexpr int RS_MAX_CLIPS = 64;          // clips per launch (their descriptors are kernel arguments)
constexpr int RS_MAX_CH = 8;

struct RsClip {
  long off;        // first sample of the clip in the flat buffer
  int n_frames;    // frames present
  int channels;
  int sr_in;
  int n_valid;     // min(n_out, T): outputs computed, the rest of the row is zero
  int step;        // table stride per input sample: int(scale * nb)
  int wing;        // most taps of one wing: (nwin - 1) / step + 1
  int stride;      // odd: lane j of a tile takes output (j * stride) mod RS_TILE (rs_stride)
  int pad_;
};
struct RsBatch { RsClip c[RS_MAX_CLIPS]; };

// The odd stride q < RS_TILE whose step in table phase, q * sr_in mod sr_out, is circularly the
// smallest non-zero one (1 when every output has the same phase): consecutive lanes then read
// neighbouring table entries.  44.1 -> 32 kHz: q = 119 moves the phase by 1 / 320 of a sample,
// so the 64 lanes of a wave read within a fifth of one table step instead of all over it.
inline int rs_stride(int sr_in, int sr_out) {
  int best = 1;
  long bestd = -1;
  for (int q = 1; q < RS_TILE; q += 2) {
    const long m = (long)q * sr_in % sr_out;
    const long d = std::min(m, (long)sr_out - m);
    if (d > 0 && (bestd < 0 || d < bestd)) { bestd = d; best = q; }
  }
  return best;
}

template <bool S16>
__device__ __forceinline__ float rs_sample(const void* frames, long i) {
  if (S16) return (float)static_cast<const short*>(frames)[i] * (1.0f / 32768.0f);   // exact
  return static_cast<const float*>(frames)[i];
}

// np.mean over the C channels of one frame as numpy sums them in float32: in order for C < 8,
// the 8-accumulator pairwise tree for C == 8; then one division by C.
template <bool S16>
__device__ __forceinline__ float rs_downmix(const void* frames, long base, int C) {
  if (C == 1) return rs_sample<S16>(frames, base);
  float s;
  if (C == RS_MAX_CH) {
    float v[RS_MAX_CH];
#pragma unroll
    for (int c = 0; c < RS_MAX_CH; ++c) v[c] = rs_sample<S16>(frames, base + c);
    s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  } else {
    s = rs_sample<S16>(frames, base);
    for (int c = 1; c < C; ++c) s += rs_sample<S16>(frames, base + c);
  }
  return __fdiv_rn(s, (float)C);
}

// One wing of the filter: sum over i < count of (win + eta * delta)[i * step] * x[DIR * i], in
// four interleaved partial sums (independent FMA chains; the rounding error of the sum stays
// well below that of one float32 chain over the same taps).
template <int DIR>
__device__ __forceinline__ float rs_wing(const float2* __restrict__ tp, int step, float eta,
                                         const float* x, int count) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = 0;
  for (; i + 4 <= count; i += 4) {
    const float2 w0 = tp[(long)i * step], w1 = tp[(long)(i + 1) * step];
    const float2 w2 = tp[(long)(i + 2) * step], w3 = tp[(long)(i + 3) * step];
    a0 = fmaf(fmaf(eta, w0.y, w0.x), x[DIR * i], a0);
    a1 = fmaf(fmaf(eta, w1.y, w1.x), x[DIR * (i + 1)], a1);
    a2 = fmaf(fmaf(eta, w2.y, w2.x), x[DIR * (i + 2)], a2);
    a3 = fmaf(fmaf(eta, w3.y, w3.x), x[DIR * (i + 3)], a3);
  }
  for (; i < count; ++i) {
    const float2 w0 = tp[(long)i * step];
    a0 = fmaf(fmaf(eta, w0.y, w0.x), x[DIR * i], a0);
  }
  return (a0 + a1) + (a2 + a3);
}

template <bool S16>
__global__ __launch_bounds__(256) void resample_pack_kernel(
    const void* __restrict__ frames, const RsBatch batch, int b0, int sr_out, int T,
    const float2* __restrict__ table, int nwin, int nb, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rs_x[];
  const RsClip& cl = batch.c[blockIdx.y];
  const long off = cl.off;
  const int n_frames = cl.n_frames, C = cl.channels, sr_in = cl.sr_in, n_valid = cl.n_valid;
  float* row = out + (long)(b0 + blockIdx.y) * T;
  const int t0 = blockIdx.x * RS_TILE;
  const int t1 = min(t0 + RS_TILE, T);
  const int tv = min(t1, n_valid);         // outputs [t0, tv) are computed, [tv, t1) are zero
  if (tv <= t0) {
    for (int t = t0 + threadIdx.x; t < t1; t += 256) row[t] = 0.f;
    return;
  }
  if (sr_in == sr_out) {                   // librosa does not resample: the downmix alone
    for (int t = t0 + threadIdx.x; t < t1; t += 256)
      row[t] = (t < tv && t < n_frames) ? rs_downmix<S16>(frames, off + (long)t * C, C) : 0.f;
    return;
  }
  const int step = cl.step, W = cl.wing;
  const int n_lo = (int)((long)t0 * sr_in / sr_out);
  const int n_hi = (int)((long)(tv - 1) * sr_in / sr_out);
  const int s0 = n_lo - W + 1;             // input sample held by rs_x[0]
  const int span = n_hi - n_lo + 2 * W;    // host: span <= the launch's LDS floats
  for (int i = threadIdx.x; i < span; i += 256) {
    const int m = s0 + i;
    rs_x[i] = (m >= 0 && m < n_frames) ? rs_downmix<S16>(frames, off + (long)m * C, C) : 0.f;
  }
  __syncthreads();
  const int D = max(sr_in, sr_out);
  const float inv_d = 1.0f / (float)D;
  const float gain = sr_out < sr_in ? (float)((double)sr_out / (double)sr_in) : 1.0f;
  // lane j takes output t0 + (j * stride mod RS_TILE): an odd stride permutes the tile, and the
  // host picks the one that puts outputs of neighbouring table phase into neighbouring lanes
  const int stride = cl.stride;
  for (int j = threadIdx.x; j < RS_TILE; j += 256) {
    const int t = t0 + ((j * stride) & (RS_TILE - 1));
    if (t >= t1) continue;
    float y = 0.f;
    if (t < tv) {
      const long p = (long)t * sr_in;
      const int n = (int)(p / sr_out), r = (int)(p % sr_out);
      const float* xc = rs_x + (n - s0);   // x[n]
      {                                    // left wing: x[n - i]
        const long ph = (long)nb * r;
        const int o = (int)(ph / D);
        const float eta = (float)(int)(ph % D) * inv_d;
        const int imax = min(n + 1, (nwin - o) / step);
        y = rs_wing<-1>(table + o, step, eta, xc, imax);
      }
      {                                    // right wing: x[n + 1 + k]
        const long ph = (long)nb * (sr_out - r);
        const int o = (int)(ph / D);
        const float eta = (float)(int)(ph % D) * inv_d;
        const int kmax = min(n_frames - n - 1, (nwin - o) / step);
        y += rs_wing<1>(table + o, step, eta, xc + 1, kmax);
      }
      y *= gain;
    }
    row[t] = y;
  }
}

// ------------------------------------------------------------------ resample into window rows
// The same signal cut into overlapping windows of one recording: window w of recording r holds
// its outputs [w * hop, w * hop + T), zero past n_out.  A sibling of resample_pack_kernel: the
// arithmetic of output t (n, r, the two table phases, the clamps imax / kmax, rs_wing, the gain)
// depends on the GLOBAL index t alone, not on the tile or the row it falls in, so a window row
// is bit-equal to the same outputs of a resample_pack row.  The window's first output g0 is a
// 64-bit quantity (p = t * sr_in already is).
struct RsRec {
  long off;        // first sample of the recording in the flat buffer
  int n_frames;    // frames present
  int channels;
  int sr_in;
  int n_out;       // outputs of the whole recording
  int step, wing, stride;   // as in RsClip
  int row0;        // first window row of the recording, relative to the launch's first row
  int n_win;
  int pad_;
};
struct RsRecBatch { RsRec c[RS_MAX_CLIPS]; };

template <bool S16>
__global__ __launch_bounds__(256) void resample_windows_kernel(
    const void* __restrict__ frames, const RsRecBatch batch, int nc, long rowbase, int y0,
    int sr_out, int T, int hop, const float2* __restrict__ table, int nwin, int nb,
    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rs_x[];
  const int wrow = y0 + blockIdx.y;        // window row within this batch of recordings
  int j = 0;                               // the recording that owns it (host: one always does)
  while (j + 1 < nc && !(wrow >= batch.c[j].row0 && wrow < batch.c[j].row0 + batch.c[j].n_win)) ++j;
  const RsRec& cl = batch.c[j];
  const long off = cl.off;
  const int n_frames = cl.n_frames, C = cl.channels, sr_in = cl.sr_in;
  const long g0 = (long)(wrow - cl.row0) * hop;   // the window's first output
  float* row = out + (rowbase + wrow) * T;
  const int t0 = blockIdx.x * RS_TILE;
  const int t1 = min(t0 + RS_TILE, T);
  // outputs [t0, tv) of the window are computed, [tv, t1) are zero
  const int tv = (int)max(0L, min((long)t1, (long)cl.n_out - g0));
  if (tv <= t0) {
    for (int t = t0 + threadIdx.x; t < t1; t += 256) row[t] = 0.f;
    return;
  }
  if (sr_in == sr_out) {                   // the downmix alone
    for (int t = t0 + threadIdx.x; t < t1; t += 256)
      row[t] = (t < tv && g0 + t < n_frames) ? rs_downmix<S16>(frames, off + (g0 + t) * C, C) : 0.f;
    return;
  }
  const int step = cl.step, W = cl.wing;
  const int n_lo = (int)((g0 + t0) * sr_in / sr_out);
  const int n_hi = (int)((g0 + tv - 1) * sr_in / sr_out);
  const int s0 = n_lo - W + 1;             // input sample held by rs_x[0]
  const int span = n_hi - n_lo + 2 * W;    // host: span <= the launch's LDS floats
  for (int i = threadIdx.x; i < span; i += 256) {
    const int m = s0 + i;
    rs_x[i] = (m >= 0 && m < n_frames) ? rs_downmix<S16>(frames, off + (long)m * C, C) : 0.f;
  }
  __syncthreads();
  const int D = max(sr_in, sr_out);
  const float inv_d = 1.0f / (float)D;
  const float gain = sr_out < sr_in ? (float)((double)sr_out / (double)sr_in) : 1.0f;
  const int stride = cl.stride;
  for (int q = threadIdx.x; q < RS_TILE; q += 256) {
    const int t = t0 + ((q * stride) & (RS_TILE - 1));
    if (t >= t1) continue;
    float y = 0.f;
    if (t < tv) {
      const long p = (g0 + t) * sr_in;
      const int n = (int)(p / sr_out), r = (int)(p % sr_out);
      const float* xc = rs_x + (n - s0);   // x[n]
      {                                    // left wing: x[n - i]
        const long ph = (long)nb * r;
        const int o = (int)(ph / D);
        const float eta = (float)(int)(ph % D) * inv_d;
        const int imax = min(n + 1, (nwin - o) / step);
        y = rs_wing<-1>(table + o, step, eta, xc, imax);
      }
      {                                    // right wing: x[n + 1 + k]
        const long ph = (long)nb * (sr_out - r);
        const int o = (int)(ph / D);
        const float eta = (float)(int)(ph % D) * inv_d;
        const int kmax = min(n_frames - n - 1, (nwin - o) / step);
        y += rs_wing<1>(table + o, step, eta, xc + 1, kmax);
      }
      y *= gain;
    }
    row[t] = y;
  }
}

}  // namespace zs

using namespace zs;

extern "C" int zs_resample_pack(const void* frames, int fmt, const long* offsets,
                                const int* n_frames, const int* channels, const int* sr_in,
                                const int* n_out, int B, int sr_out, int T, const float* table,
                                int num_zeros, int precision, float* out, void* stream) {
  ZS_REQUIRE(frames && offsets && n_frames && channels && sr_in && n_out && table && out,
             "zs_resample_pack: NULL buffer");
  ZS_REQUIRE(B > 0 && T > 0, "zs_resample_pack: B > 0, T > 0");
  ZS_REQUIRE(fmt == 0 || fmt == 1, "zs_resample_pack: fmt %d (0: f32, 1: s16)", fmt);
  ZS_REQUIRE(sr_out >= 1 && sr_out <= (1 << 24), "zs_resample_pack: 1 <= sr_out <= 2^24");
  ZS_REQUIRE(num_zeros >= 1 && num_zeros <= 1024 && precision >= 0 && precision <= 12,
             "zs_resample_pack: 1 <= num_zeros <= 1024, 0 <= precision <= 12");
  ZS_REQUIRE(((uintptr_t)table & 7) == 0, "zs_resample_pack: table 8-byte aligned");
  const int nb = 1 << precision, nwin = nb * num_zeros + 1;
  // every clip is checked before the first launch
  for (int b = 0; b < B; ++b) {
    ZS_REQUIRE(channels[b] >= 1 && channels[b] <= RS_MAX_CH,
               "zs_resample_pack: clip %d has %d channels (1..%d)", b, channels[b], RS_MAX_CH);
    ZS_REQUIRE(sr_in[b] >= 1 && sr_in[b] <= (1 << 24), "zs_resample_pack: clip %d: 1 <= sr_in <= 2^24", b);
    ZS_REQUIRE((long)sr_in[b] <= 8L * sr_out && (long)sr_out <= 8L * sr_in[b],
               "zs_resample_pack: clip %d: %d Hz -> %d Hz is beyond a factor of 8", b, sr_in[b], sr_out);
    ZS_REQUIRE(n_frames[b] >= 0 && n_out[b] >= 0 && offsets[b] >= 0,
               "zs_resample_pack: clip %d: negative length or offset", b);
    ZS_REQUIRE((long)T * sr_in[b] / sr_out < 0x7fffffffL,
               "zs_resample_pack: clip %d: T * sr_in / sr_out does not fit an int", b);
    const int step = sr_out < sr_in[b] ? (int)((long)nb * sr_out / sr_in[b]) : nb;
    ZS_REQUIRE(step >= 1, "zs_resample_pack: clip %d: table step 0 (precision %d too low for %d Hz -> %d Hz)",
               b, precision, sr_in[b], sr_out);
    const long span = (long)(RS_TILE - 1) * sr_in[b] / sr_out + 2L * ((nwin - 1) / step + 1) + 2;
    ZS_REQUIRE(span * 4 <= 65536, "zs_resample_pack: clip %d: a tile's input span (%ld floats) exceeds 64 KB of LDS", b, span);
  }
  for (int b0 = 0; b0 < B; b0 += RS_MAX_CLIPS) {
    const int nc = std::min(RS_MAX_CLIPS, B - b0);
    RsBatch batch = {};
    long lds = 0;
    for (int j = 0; j < nc; ++j) {
      const int b = b0 + j;
      RsClip& c = batch.c[j];
      c.off = offsets[b];
      c.n_frames = n_frames[b];
      c.channels = channels[b];
      c.sr_in = sr_in[b];
      c.n_valid = std::min(n_out[b], T);
      c.step = sr_out < sr_in[b] ? (int)((long)nb * sr_out / sr_in[b]) : nb;
      c.wing = (nwin - 1) / c.step + 1;
      c.stride = rs_stride(sr_in[b], sr_out);
      if (sr_in[b] != sr_out)
        lds = std::max(lds, (long)(RS_TILE - 1) * sr_in[b] / sr_out + 2L * c.wing + 2);
    }
    const dim3 grid(cdiv(T, RS_TILE), nc);
    const float2* tab = reinterpret_cast<const float2*>(table);
    if (fmt == 1)
      hipLaunchKernelGGL(resample_pack_kernel<true>, grid, dim3(256), lds * sizeof(float), S(stream),
                         frames, batch, b0, sr_out, T, tab, nwin, nb, out);
    else
      hipLaunchKernelGGL(resample_pack_kernel<false>, grid, dim3(256), lds * sizeof(float), S(stream),
                         frames, batch, b0, sr_out, T, tab, nwin, nb, out);
    ZS_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int zs_resample_windows(const void* frames, int fmt, const long* offsets,
                                   const int* n_frames, const int* channels, const int* sr_in,
                                   const int* n_out, const int* n_win, int R, int sr_out, int T,
                                   int hop, const float* table, int num_zeros, int precision,
                                   float* out, void* stream) {
  ZS_REQUIRE(frames && offsets && n_frames && channels && sr_in && n_out && n_win && table && out,
             "zs_resample_windows: NULL buffer");
  ZS_REQUIRE(R > 0 && T > 0, "zs_resample_windows: R > 0, T > 0");
  ZS_REQUIRE(hop > 0, "zs_resample_windows: hop > 0");
  ZS_REQUIRE(fmt == 0 || fmt == 1, "zs_resample_windows: fmt %d (0: f32, 1: s16)", fmt);
  ZS_REQUIRE(sr_out >= 1 && sr_out <= (1 << 24), "zs_resample_windows: 1 <= sr_out <= 2^24");
  ZS_REQUIRE(num_zeros >= 1 && num_zeros <= 1024 && precision >= 0 && precision <= 12,
             "zs_resample_windows: 1 <= num_zeros <= 1024, 0 <= precision <= 12");
  ZS_REQUIRE(((uintptr_t)table & 7) == 0, "zs_resample_windows: table 8-byte aligned");
  const int nb = 1 << precision, nwin = nb * num_zeros + 1;
  // every recording is checked before the first launch
  long rows = 0;
  for (int b = 0; b < R; ++b) {
    ZS_REQUIRE(channels[b] >= 1 && channels[b] <= RS_MAX_CH,
               "zs_resample_windows: recording %d has %d channels (1..%d)", b, channels[b], RS_MAX_CH);
    ZS_REQUIRE(sr_in[b] >= 1 && sr_in[b] <= (1 << 24),
               "zs_resample_windows: recording %d: 1 <= sr_in <= 2^24", b);
    ZS_REQUIRE((long)sr_in[b] <= 8L * sr_out && (long)sr_out <= 8L * sr_in[b],
               "zs_resample_windows: recording %d: %d Hz -> %d Hz is beyond a factor of 8", b, sr_in[b], sr_out);
    ZS_REQUIRE(n_frames[b] >= 0 && n_out[b] >= 0 && offsets[b] >= 0,
               "zs_resample_windows: recording %d: negative length or offset", b);
    ZS_REQUIRE(n_win[b] >= 0, "zs_resample_windows: recording %d: n_win %d < 0", b, n_win[b]);
    ZS_REQUIRE(n_win[b] <= 1 || (long)(n_win[b] - 1) * hop < (long)std::max(n_out[b], 1),
               "zs_resample_windows: recording %d: window %d starts at output %ld of %d (no valid output)",
               b, n_win[b] - 1, (long)(n_win[b] - 1) * hop, n_out[b]);
    ZS_REQUIRE((long)T * sr_in[b] / sr_out < 0x7fffffffL,
               "zs_resample_windows: recording %d: T * sr_in / sr_out does not fit an int", b);
    ZS_REQUIRE((long)n_out[b] * sr_in[b] / sr_out < 0x7fffffffL,
               "zs_resample_windows: recording %d: n_out * sr_in / sr_out does not fit an int", b);
    const int step = sr_out < sr_in[b] ? (int)((long)nb * sr_out / sr_in[b]) : nb;
    ZS_REQUIRE(step >= 1, "zs_resample_windows: recording %d: table step 0 (precision %d too low for %d Hz -> %d Hz)",
               b, precision, sr_in[b], sr_out);
    const long span = (long)(RS_TILE - 1) * sr_in[b] / sr_out + 2L * ((nwin - 1) / step + 1) + 2;
    ZS_REQUIRE(span * 4 <= 65536, "zs_resample_windows: recording %d: a tile's input span (%ld floats) exceeds 64 KB of LDS", b, span);
    rows += n_win[b];
    ZS_REQUIRE(rows < 0x7fffffffL && rows <= 0x7fffffffffffffffL / T,
               "zs_resample_windows: sum n_win (an int) times T does not fit a long");
  }
  long rowbase = 0;
  for (int b0 = 0; b0 < R; b0 += RS_MAX_CLIPS) {
    const int nc = std::min(RS_MAX_CLIPS, R - b0);
    RsRecBatch batch = {};
    long lds = 0, nrows = 0;
    for (int j = 0; j < nc; ++j) {
      const int b = b0 + j;
      RsRec& c = batch.c[j];
      c.off = offsets[b];
      c.n_frames = n_frames[b];
      c.channels = channels[b];
      c.sr_in = sr_in[b];
      c.n_out = n_out[b];
      c.step = sr_out < sr_in[b] ? (int)((long)nb * sr_out / sr_in[b]) : nb;
      c.wing = (nwin - 1) / c.step + 1;
      c.stride = rs_stride(sr_in[b], sr_out);
      c.row0 = (int)nrows;
      c.n_win = n_win[b];
      nrows += n_win[b];
      if (sr_in[b] != sr_out)
        lds = std::max(lds, (long)(RS_TILE - 1) * sr_in[b] / sr_out + 2L * c.wing + 2);
    }
    const float2* tab = reinterpret_cast<const float2*>(table);
    for (long y0 = 0; y0 < nrows; y0 += 65535) {       // grid.y holds at most 65535 rows
      const dim3 grid(cdiv(T, RS_TILE), (unsigned)std::min(65535L, nrows - y0));
      if (fmt == 1)
        hipLaunchKernelGGL(resample_windows_kernel<true>, grid, dim3(256), lds * sizeof(float), S(stream),
                           frames, batch, nc, rowbase, (int)y0, sr_out, T, hop, tab, nwin, nb, out);
      else
        hipLaunchKernelGGL(resample_windows_kernel<false>, grid, dim3(256), lds * sizeof(float), S(stream),
                           frames, batch, nc, rowbase, (int)y0, sr_out, T, hop, tab, nwin, nb, out);
      ZS_LAUNCH_CHECK();
    }
    rowbase += nrows;
  }
  return 0;
}

extern "C" int zs_pack_clips(const float* flat, const long* offsets, const int* lengths, int B,
                             int T, float* out, void* stream) {
  ZS_REQUIRE(B > 0 && T > 0 && T % 4 == 0, "zs_pack_clips: B > 0, T > 0, T %% 4 == 0");
  ZS_REQUIRE(flat && offsets && lengths && out && ((uintptr_t)out & 15) == 0,
             "zs_pack_clips: pointers (out 16-byte aligned)");
  hipLaunchKernelGGL(pack_clips_kernel, dim3(std::min(cdiv(T, 1024), 64), B), dim3(256), 0,
                     S(stream), flat, offsets, lengths, T, out);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_logmel(const float* wav, int B, int T, const float* window, const float* twiddle,
                         const float* melW, const int* mel_lo, const int* mel_hi,
                         const float* bn_mean, const float* bn_var, const float* bn_weight,
                         const float* bn_bias, float* out, void* stream) {
  ZS_REQUIRE(B > 0 && T > NFFT / 2, "zs_logmel: need T > 512 samples for reflect padding");
  ZS_REQUIRE(wav && window && twiddle && melW && mel_lo && mel_hi && out, "zs_logmel: NULL buffer");
  ZS_REQUIRE(!bn_mean || (bn_var && bn_weight && bn_bias), "zs_logmel: bn0 needs all four vectors");
  ZS_REQUIRE((long)B * (T / HOP + 1) <= 0x7fffffffL, "zs_logmel: B * n_frames does not fit an int");
  const int n_frames = T / HOP + 1;
  const int total = B * n_frames;
  if (g_logmel_wave) {
    const int npairs = cdiv(total, 2);
    // 3 blocks per CU fit the LDS (47.6 KB each): one resident wave of blocks, no tail round
    hipLaunchKernelGGL(logmel_wave_kernel, dim3(std::min(cdiv(npairs, 4), 256 * 3)), dim3(256), 0,
                       S(stream), wav, T, n_frames, total, window, twiddle, melW, mel_lo, mel_hi,
                       bn_mean, bn_var, bn_weight, bn_bias, out);
    ZS_LAUNCH_CHECK();
    return 0;
  }
  const int groups = cdiv(total, 2 * LM_PAIRS);
  hipLaunchKernelGGL(logmel_kernel, dim3(std::min(groups, 256 * 8)), dim3(256), 0, S(stream), wav, T,
                     n_frames, total, window, twiddle, melW, mel_lo, mel_hi, bn_mean, bn_var,
                     bn_weight, bn_bias, out);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_wav2img(const float* in, int B, int T_in, float* img, void* stream) {
  ZS_REQUIRE(B > 0 && T_in > 1 && T_in <= 1024, "zs_wav2img: B > 0, 1 < T_in <= 1024");
  ZS_REQUIRE(in && img, "zs_wav2img: NULL buffer");
  ZS_REQUIRE(B <= 0x7fffffff / 65536, "zs_wav2img: B * 65536 does not fit an int");
  const long total = (long)B * 65536;
  hipLaunchKernelGGL(wav2img_kernel, dim3(cdiv(total, 256)), dim3(256), 0, S(stream), in, T_in, img);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_patch_embed(const float* img, int B, const float* w, const float* b,
                              const float* ln_w, const float* ln_b, float* x, void* stream) {
  ZS_REQUIRE(B > 0 && B <= 0x7fffffff / 65536, "zs_patch_embed: B > 0, B * 65536 fits an int");
  ZS_REQUIRE(img && w && b && ln_w && ln_b && x, "zs_patch_embed: NULL buffer");
  const long ntok = (long)B * 4096;
  hipLaunchKernelGGL(patch_embed_kernel, dim3(cdiv(ntok, 64)), dim3(256), 0, S(stream), img, w, b,
                     ln_w, ln_b, x, ntok);
  ZS_LAUNCH_CHECK();
  return 0;
}
