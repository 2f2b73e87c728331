// The HTSAT tagging head (htsat.py:830-894): clip-level tags and frame-level sound events from the
// last stage's tokens, the tensor zs_ln_meanpool reads.
//   tag_prep_kernel   final LayerNorm of the 64 tokens of a clip -> xn (the conv's operand, engine
//                     dtype) and fine[tau] = the mean of a frame's two frequency bins (f32)
//   tag_conv_kernel   tscam_conv = Conv2d(C, N, (2, 3), padding (0, 1)) as an implicit GEMM with a
//                     gathered A operand, + bias, sigmoid per frame, sigmoid of the time mean per clip
//
// Token n = f * 8 + t (frequency row f, time column t).  htsat.py:834-839 regroups the 8 x 8 map
// into 32 time frames tau = 8 g + t of 2 frequency bins c, f = 2 g + c:
//   tok(tau, c) = (2 (tau / 8) + c) * 8 + tau % 8
// so frames 7 and 8 are neighbours in time although they come from different token rows.
//
// The GEMM: M = 32 frames of ONE clip per workgroup (the time mean is tile-local: no atomics),
// 128 classes per workgroup (4 waves x 2 n-tiles of 16), K = 6 C in the order (c, d, ch).  C is a
// multiple of 32, so a k-step of 32 lies inside one (c, d) tap and the A fragment of frame tau is
// 32 channels of token tok(tau + d - 1, c) -- read straight from xn (a clip's 64 rows stay in
// L1 / L2), zero where tau + d - 1 leaves [0, 32).  No im2col matrix exists anywhere.  The weight
// is fragment-packed as for swin.hip: frag(nt, ks)[lane][j] = W[16 nt + lane % 16][32 ks + 8 (lane
// / 16) + j], [N/16][K/32][64][8], one contiguous wave-load per fragment (1 KiB bf16, 2 KiB f32).
//   bf16: v_mfma_f32_16x16x32_bf16, one per fragment;
//   f32:  v_mfma_f32_16x16x4_f32, eight per fragment, MFMA j taking element j of every lane
//         (exact f32 products, f32 accumulation).
// Every column runs the same chain of MFMAs in the same order whatever its n-tile, clip or batch,
// and the time mean is one fixed tree: results do not depend on B or on the clip's neighbours,
// and two equal weight rows give bit-equal columns.
#include "common.h"

namespace zs {

typedef __attribute__((ext_vector_type(8))) __bf16 tg_bf16x8;
typedef __attribute__((ext_vector_type(4))) float tg_f32x4;

__device__ __forceinline__ int tag_tok(int tau, int c) { return (2 * (tau >> 3) + c) * 8 + (tau & 7); }

// one wave per (clip, frame): the frame's two tokens in registers (CPL values per lane each)
template <int CPL, typename TO>
__global__ __launch_bounds__(256) void tag_prep_kernel(const float* __restrict__ x, int B, int C,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ b,
                                                       TO* __restrict__ xn,
                                                       float* __restrict__ fine) {
  const int lane = threadIdx.x & 63;
  const int fr = blockIdx.x * 4 + (threadIdx.x >> 6);     // clip * 32 + tau
  if (fr >= B * 32) return;
  const int clip = fr >> 5, tau = fr & 31;
  float v[2][CPL];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const long row = (long)clip * 64 + tag_tok(tau, c);
    const float* xr = x + row * C;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int ch = lane + 64 * q;
      v[c][q] = ch < C ? xr[ch] : 0.f;
      s += v[c][q];
    }
    const float mean = wave_sum(s) / C;
    float d2 = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const float d = lane + 64 * q < C ? v[c][q] - mean : 0.f;
      d2 += d * d;
    }
    const float rstd = rsqrtf(wave_sum(d2) / C + 1e-5f);
    TO* yr = xn + row * C;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int ch = lane + 64 * q;
      if (ch < C) {
        v[c][q] = (v[c][q] - mean) * rstd * w[ch] + b[ch];
        stf(yr + ch, v[c][q]);
      }
    }
  }
  float* fo = fine + (long)fr * C;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int ch = lane + 64 * q;
    if (ch < C) fo[ch] = (v[0][q] + v[1][q]) * 0.5f;   // from the f32 xn, before any rounding
  }
}

// the operand of one k-step: 32 channels of a token row, 8 per lane group (lane / 16)
template <typename T> struct TagFrag;
template <> struct TagFrag<bf16_t> {
  uint4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void zero_unless(bool keep) {
    if (!keep) v = make_uint4(0, 0, 0, 0);
  }
  static __device__ __forceinline__ tg_f32x4 mma(const TagFrag& a, const TagFrag& w, tg_f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tg_bf16x8, a.v),
                                                   __builtin_bit_cast(tg_bf16x8, w.v), acc, 0, 0, 0);
  }
};
template <> struct TagFrag<float> {
  float4 lo, hi;
  __device__ __forceinline__ void load(const float* p) {
    lo = *reinterpret_cast<const float4*>(p);
    hi = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void zero_unless(bool keep) {
    if (!keep) lo = hi = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  static __device__ __forceinline__ tg_f32x4 mma(const TagFrag& a, const TagFrag& w, tg_f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.x, w.lo.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.y, w.lo.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.z, w.lo.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.w, w.lo.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.x, w.hi.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.y, w.hi.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.z, w.hi.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.w, w.hi.w, acc, 0, 0, 0);
    return acc;
  }
};

__device__ __forceinline__ float tag_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// grid (ceil(N / 128), B), 256 threads.  Wave w owns n-tiles 8 blockIdx.x + 2 w + {0, 1}; a tile
// past the last one is skipped (wave-uniform).  acc[mi][j][i]: frame 16 mi + 4 (lane / 16) + i,
// class 16 nt_j + lane % 16.
template <typename T>
__global__ __launch_bounds__(256) void tag_conv_kernel(const T* __restrict__ xn, int C, int N,
                                                       const T* __restrict__ wp,
                                                       const float* __restrict__ bias,
                                                       float* __restrict__ frame, int ldf,
                                                       float* __restrict__ clip, int ldc,
                                                       float* __restrict__ logits) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int ntiles = (N + 15) >> 4, ksc = C >> 5, kstot = 6 * ksc;
  const int nt0 = blockIdx.x * 8 + wid * 2;
  if (nt0 >= ntiles) return;
  const bool two = nt0 + 1 < ntiles;
  const int b = blockIdx.y;
  const T* xb = xn + (long)b * 64 * C + 8 * g;
  const T* w0 = wp + ((long)nt0 * kstot * 64 + lane) * 8;
  const T* w1 = two ? w0 + (long)kstot * 64 * 8 : w0;
  tg_f32x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[mi][j] = (tg_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int cd = 0; cd < 6; ++cd) {
    const int c = cd / 3, d = cd - 3 * c;
    const T* ar[2];
    bool ok[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int ts = 16 * mi + l16 + d - 1;            // the source frame of this tap
      ok[mi] = ts >= 0 && ts < 32;
      ar[mi] = xb + (long)tag_tok(ok[mi] ? ts : 0, c) * C;   // padding lanes read a valid row
    }
    const T* wk0 = w0 + (long)cd * ksc * 512;
    const T* wk1 = w1 + (long)cd * ksc * 512;
    // U k-steps of fragments are requested before the first of their MFMAs (the loads are L2
    // round trips); the MFMAs run in k order whatever U is, so U does not change a bit
    constexpr int U = sizeof(T) == 2 ? 4 : 2;
    for (int ks0 = 0; ks0 < ksc; ks0 += U) {
      TagFrag<T> a[U][2], w[U][2];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ks0 + u < ksc) {
#pragma unroll
          for (int mi = 0; mi < 2; ++mi) a[u][mi].load(ar[mi] + 32 * (ks0 + u));
          w[u][0].load(wk0 + (long)(ks0 + u) * 512);
          w[u][1].load(wk1 + (long)(ks0 + u) * 512);
        }
      // f32: the f32 MFMA is one fmaf chain per output, and a single chain over K = 4608 loses
      // about eps sqrt(K) / 2 of the result; the U k-steps (64 products) go into a fresh
      // accumulator that is then added to the total, two levels of short chains (measured
      // against float64 on the 768-channel cases: 1.4e-5 in one chain, at a float32 yardstick
      // of 1.7e-6).  bf16 operands: the operand rounding dominates, one chain.
      constexpr bool TWO_LEVEL = sizeof(T) == 4;
      tg_f32x4 part[2][2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          part[mi][j] = TWO_LEVEL ? (tg_f32x4){0.f, 0.f, 0.f, 0.f} : acc[mi][j];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ks0 + u < ksc) {
#pragma unroll
          for (int mi = 0; mi < 2; ++mi) {
            a[u][mi].zero_unless(ok[mi]);
            part[mi][0] = TagFrag<T>::mma(a[u][mi], w[u][0], part[mi][0]);
            part[mi][1] = TagFrag<T>::mma(a[u][mi], w[u][1], part[mi][1]);
          }
        }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[mi][j] = TWO_LEVEL ? acc[mi][j] + part[mi][j] : part[mi][j];
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = (nt0 + j) * 16 + l16;
    const bool real = (j == 0 || two) && n < N;
    const float bv = real ? bias[n] : 0.f;
    float s[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      float z[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        z[i] = acc[mi][j][i] + bv;
        if (real) {
          const long o = ((long)b * 32 + 16 * mi + 4 * g + i) * ldf + n;
          frame[o] = tag_sigmoid(z[i]);
          if (logits) logits[o] = z[i];
        }
      }
      s[mi] = (z[0] + z[1]) + (z[2] + z[3]);
    }
    // the time mean: 8 frames per lane, then the 4 lane groups, one fixed tree
    float t = s[0] + s[1];
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (real && g == 0) clip[(long)b * ldc + n] = tag_sigmoid(t * (1.0f / 32.0f));
  }
}

}  // namespace zs

using namespace zs;

extern "C" int zs_tag_prep(const float* x, int B, int C, const float* ln_w, const float* ln_b,
                           void* xn, int dtype, float* fine, void* stream) {
  ZS_REQUIRE(B > 0 && C > 0 && C % 32 == 0 && C <= 2048,
             "zs_tag_prep: bad shape (B > 0, C a multiple of 32, C <= 2048)");
  ZS_REQUIRE((long)B * 64 <= 0x7fffffffL / 64, "zs_tag_prep: B too large");
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "zs_tag_prep: dtype");
  ZS_REQUIRE(x && ln_w && ln_b && xn && fine, "zs_tag_prep: NULL buffer");
  const dim3 grid(cdiv((long)B * 32, 4));
#define TGP(CPL_)                                                                                 \
  do {                                                                                            \
    if (dtype == ZS_BF16)                                                                         \
      hipLaunchKernelGGL((tag_prep_kernel<CPL_, bf16_t>), grid, dim3(256), 0, S(stream), x, B, C, \
                         ln_w, ln_b, (bf16_t*)xn, fine);                                          \
    else                                                                                          \
      hipLaunchKernelGGL((tag_prep_kernel<CPL_, float>), grid, dim3(256), 0, S(stream), x, B, C,  \
                         ln_w, ln_b, (float*)xn, fine);                                           \
  } while (0)
  if (C <= 256) TGP(4); else if (C <= 768) TGP(12); else TGP(32);
#undef TGP
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_tag_conv(const void* xn, int B, int C, int dtype, const void* w_packed, int N,
                           const float* bias, float* frame, int ldf, float* clip, int ldc,
                           float* logits, void* stream) {
  ZS_REQUIRE(B > 0 && B <= 65535 && C > 0 && C % 32 == 0 && C <= 2048,
             "zs_tag_conv: bad shape (0 < B <= 65535, C a multiple of 32, C <= 2048)");
  ZS_REQUIRE(N > 0 && N <= (1 << 20), "zs_tag_conv: N must be in 1 .. 2^20");
  ZS_REQUIRE(ldf >= N && ldc >= N, "zs_tag_conv: ldf and ldc must be at least N");
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "zs_tag_conv: dtype");
  ZS_REQUIRE(xn && w_packed && bias && frame && clip, "zs_tag_conv: NULL buffer");
  ZS_REQUIRE(((uintptr_t)xn & 15) == 0 && ((uintptr_t)w_packed & 15) == 0,
             "zs_tag_conv: xn and w_packed must be 16-byte aligned");
  const dim3 grid(cdiv(N, 128), B);
  if (dtype == ZS_BF16)
    hipLaunchKernelGGL(tag_conv_kernel<bf16_t>, grid, dim3(256), 0, S(stream), (const bf16_t*)xn, C,
                       N, (const bf16_t*)w_packed, bias, frame, ldf, clip, ldc, logits);
  else
    hipLaunchKernelGGL(tag_conv_kernel<float>, grid, dim3(256), 0, S(stream), (const float*)xn, C, N,
                       (const float*)w_packed, bias, frame, ldf, clip, ldc, logits);
  ZS_LAUNCH_CHECK();
  return 0;
}
