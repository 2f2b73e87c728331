// Training of the MLP prefix mapper with GPT-2 frozen: the backward kernels behind
// the teacher-forced cross-entropy (train_prompt.py:133 over ClapCaption_prompt.forward,
// caption_model.py:297-313), AdamW and the training-side noise_injection (utils.py:19-31).
// Every product that is a matrix product stays zs_gemm (on transposed weight copies made by
// transpose_cast_kernel); this file holds what is not a GEMM.  Nothing here is atomic and every
// reduction runs in a fixed order, so results are bit-identical from run to run.
#include "common.h"
#include <math.h>

namespace zs {
namespace tr {

// 8 consecutive values as floats (one 16-byte load for bf16, two for f32; p aligned to 16 bytes)
__device__ __forceinline__ void load8(const float* p, float* o) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void load8(const bf16_t* p, float* o) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
// row . vec: 64 values of a global row against 64 floats in LDS (broadcast reads)
template <typename T>
__device__ __forceinline__ float dot64(const T* __restrict__ row, const float* vec) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float r[8];
    load8(row + 8 * c, r);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(r[e], vec[8 * c + e], acc);
  }
  return acc;
}

// ---------------------------------------------------------------- attention backward
// One workgroup of 4 waves per (head, clip).  Pass 1 walks the query rows (wave w: rows w, w+4,
// ..): lane l holds keys l, l+64, l+128, l+192 of the row's scores s = q.k/8 and dP = dO.v,
// reduces the row's log-sum-exp and D = sum_j P dP over the wave, leaves dS = P (dP - D) in LDS
// and then, as lane = head column, adds dQ[d] = sum_j dS_j K[j][d] / 8 in key order.  lse and D of
// every row stay in LDS.  Pass 2 walks the key rows the same way over the queries i >= j,
// recomputing P and dS from the stored lse / D, and adds dV[d] = sum_i P_i dO[i][d] and
// dK[d] = sum_i dS_i Q[i][d] / 8 in query order: dK / dV of a (clip, head) are accumulated inside
// this one workgroup in a fixed order.  Rows >= len are never read and get zeros.
// Correct and deterministic, not fast: every lane walks its own K / V / Q / dO row (16-byte loads
// 3*heads*64 elements apart between lanes, nothing coalesced) and the dQ / dK / dV sums are serial
// per-wave loops with one global load per iteration, so the kernel is latency-bound -- 126 us per
// layer at B 40, L 45, 12 heads in bf16, the largest kernel of the step.  An MFMA
// version on K / V tiles staged in LDS is the follow-up.
template <typename T>
__global__ __launch_bounds__(256) void attention_bwd_kernel(const T* __restrict__ qkv,
                                                            const T* __restrict__ dO, int L,
                                                            const int* __restrict__ lens, int heads,
                                                            T* __restrict__ dqkv) {
  __shared__ float s_lse[256], s_D[256];
  __shared__ float s_p[4][256], s_ds[4][256];
  __shared__ float s_x[4][64], s_y[4][64];
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ldo = heads * 64, ld = 3 * ldo;
  const int len = min(max(lens ? lens[b] : L, 0), L);
  const T* Q = qkv + (long)b * L * ld + h * 64;
  const T* K = Q + ldo;
  const T* V = K + ldo;
  const T* DO = dO + (long)b * L * ldo + h * 64;
  T* DQ = dqkv + (long)b * L * ld + h * 64;
  T* DK = DQ + ldo;
  T* DV = DK + ldo;
  for (int i = len + w; i < L; i += 4) {
    stf(DQ + (long)i * ld + lane, 0.f);
    stf(DK + (long)i * ld + lane, 0.f);
    stf(DV + (long)i * ld + lane, 0.f);
  }
  // ---- pass 1: per query row
  for (int i0 = 0; i0 < len; i0 += 4) {
    const int i = i0 + w;
    const bool on = i < len;
    if (on) {
      s_x[w][lane] = ldf(Q + (long)i * ld + lane);
      s_y[w][lane] = ldf(DO + (long)i * ldo + lane);
    }
    __syncthreads();
    if (on) {
      float s[4], dp[4], mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = lane + 64 * t;
        s[t] = -INFINITY;
        dp[t] = 0.f;
        if (j <= i) {
          s[t] = 0.125f * dot64(K + (long)j * ld, s_x[w]);
          dp[t] = dot64(V + (long)j * ld, s_y[w]);
          mx = fmaxf(mx, s[t]);
        }
      }
      mx = wave_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (lane + 64 * t <= i) sum += expf(s[t] - mx);
      const float lse = mx + logf(wave_sum(sum));
      float p[4], dd = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        p[t] = lane + 64 * t <= i ? expf(s[t] - lse) : 0.f;
        dd = fmaf(p[t], dp[t], dd);
      }
      dd = wave_sum(dd);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (lane + 64 * t <= i) s_ds[w][lane + 64 * t] = p[t] * (dp[t] - dd);
      if (lane == 0) {
        s_lse[i] = lse;
        s_D[i] = dd;
      }
    }
    __syncthreads();
    if (on) {
      float acc = 0.f;
      for (int j = 0; j <= i; ++j) acc = fmaf(s_ds[w][j], ldf(K + (long)j * ld + lane), acc);
      stf(DQ + (long)i * ld + lane, 0.125f * acc);
    }
  }
  __syncthreads();
  // ---- pass 2: per key row
  for (int j0 = 0; j0 < len; j0 += 4) {
    const int j = j0 + w;
    const bool on = j < len;
    if (on) {
      s_x[w][lane] = ldf(K + (long)j * ld + lane);
      s_y[w][lane] = ldf(V + (long)j * ld + lane);
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = j + lane + 64 * t;
        if (i < len) {
          const float s = 0.125f * dot64(Q + (long)i * ld, s_x[w]);
          const float dp = dot64(DO + (long)i * ldo, s_y[w]);
          const float p = expf(s - s_lse[i]);
          s_p[w][i - j] = p;
          s_ds[w][i - j] = p * (dp - s_D[i]);
        }
      }
    }
    __syncthreads();
    if (on) {
      float av = 0.f, ak = 0.f;
      for (int i = j; i < len; ++i) {
        av = fmaf(s_p[w][i - j], ldf(DO + (long)i * ldo + lane), av);
        ak = fmaf(s_ds[w][i - j], ldf(Q + (long)i * ld + lane), ak);
      }
      stf(DV + (long)j * ld + lane, av);
      stf(DK + (long)j * ld + lane, 0.125f * ak);
    }
  }
}

// ---------------------------------------------------------------- LayerNorm backward
// One wave per row (two-pass mean / variance as layernorm_kernel):  xhat = (x - mean) rstd,
// a = dy g,  dx = rstd (a - mean(a) - xhat mean(a xhat)) (+ res).  rows != NULL: row m of dy
// belongs to row rows[m] of x / res / dx.
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(
    const float* __restrict__ x, int M, int C, int ldx, const int* __restrict__ rows,
    const float* __restrict__ dy, int ldy, const float* __restrict__ g, float eps, const float* res,
    int ldr, float* dx, int ldd) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const long r = rows ? rows[m] : m;
  const float* xr = x + r * ldx;
  const float* dyr = dy + (long)m * ldy;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mean = wave_sum(s) / C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - mean;
    v += d * d;
  }
  const float rstd = rsqrtf(wave_sum(v) / C + eps);
  float sa = 0.f, sb = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float a = dyr[c] * (g ? g[c] : 1.f);
    sa += a;
    sb = fmaf(a, (xr[c] - mean) * rstd, sb);
  }
  const float ma = wave_sum(sa) / C, mb = wave_sum(sb) / C;
  const float* rr = res ? res + r * ldr : nullptr;
  float* dr = dx + r * ldd;
  for (int c = lane; c < C; c += 64) {
    const float a = dyr[c] * (g ? g[c] : 1.f);
    const float o = rstd * (a - ma - (xr[c] - mean) * rstd * mb);
    dr[c] = rr ? rr[c] + o : o;
  }
}

// ---------------------------------------------------------------- activations
// gelu_new'(u) = 0.5 (1 + t) + 0.5 u (1 - t^2) c (1 + 3 * 0.044715 u^2),  t = tanh(c (u + 0.044715 u^3))
template <typename T>
__global__ void gelu_tanh_bwd_kernel(const T* __restrict__ u, const float* __restrict__ dh, long n,
                                     T* __restrict__ du) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float c = 0.7978845608028654f;
  const float x = ldf(u + i);
  const float t = tanhf(c * (x + 0.044715f * x * x * x));
  const float d = 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) * c * (1.f + 0.134145f * x * x);
  stf(du + i, d * dh[i]);
}

__global__ void tanh_bwd_kernel(const float* __restrict__ h, const float* __restrict__ dh, long n,
                                float* __restrict__ dpre) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dpre[i] = (1.f - h[i] * h[i]) * dh[i];
}

// ---------------------------------------------------------------- LM-head gradient rows
// dhf[m] = w (mix[m] - wte[tgt[m]]),  w = 1 / sum_b cnt[b] (added in clip order), zeros for a
// row without a target.  One block per row.
template <typename T>
__global__ __launch_bounds__(256) void nll_grad_rows_kernel(
    const float* __restrict__ mix, int ldm, const T* __restrict__ wte, int V, int K,
    const int* __restrict__ tgt, const int* __restrict__ cnt, int B, float* __restrict__ dhf,
    int ldd) {
  const int m = blockIdx.x;
  const int t = tgt[m];
  int n = 0;
  for (int b = 0; b < B; ++b) n += cnt[b];
  const bool on = t >= 0 && t < V && n > 0;
  const float w = on ? 1.f / (float)n : 0.f;
  for (int k = threadIdx.x; k < K; k += 256)
    dhf[(long)m * ldd + k] = on ? w * (mix[(long)m * ldm + k] - ldf(wte + (long)t * K + k)) : 0.f;
}

// loss[0] = -sum_b sum[b] / sum_b cnt[b], added in clip order (NaN without tokens: 0 / 0)
__global__ void nll_loss_kernel(const float* __restrict__ sum, const int* __restrict__ cnt, int B,
                                float* __restrict__ loss) {
  if (threadIdx.x || blockIdx.x) return;
  float s = 0.f;
  int n = 0;
  for (int b = 0; b < B; ++b) {
    s += sum[b];
    n += cnt[b];
  }
  loss[0] = -s / (float)n;
}

// d_soft[b][j*D + d] = dx[(b*Smax + H_b + j)*D + d]: the residual-stream gradient at the soft rows
__global__ void soft_grad_rows_kernel(const float* __restrict__ dx, const int* __restrict__ hard_len,
                                      int h_cap, int n_soft, int Smax, int D,
                                      float* __restrict__ d_soft, int ld) {
  const int b = blockIdx.y, j = blockIdx.x;
  const int H = min(max(hard_len[b], 0), h_cap);
  const float* src = dx + ((long)b * Smax + H + j) * D;
  float* dst = d_soft + (long)b * ld + (long)j * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) dst[d] = src[d];
}

// ---------------------------------------------------------------- column sums, transposes
__global__ void colsum_kernel(const float* __restrict__ x, int B, int N, int ldx,
                              float* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += x[(long)b * ldx + n];
  out[n] = s;
}

// y[c][r] = x[r][c] for r < R, 0 for R <= r < Rp; 32 x 32 tiles through LDS
template <typename T>
__global__ __launch_bounds__(256) void transpose_cast_kernel(const float* __restrict__ x, int R,
                                                             int C, int ldx, T* __restrict__ y,
                                                             int Rp) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < R && c < C) ? x[(long)r * ldx + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (c < C && r < Rp) stf(y + (long)c * Rp + r, tile[tx][k]);
  }
}

// ---------------------------------------------------------------- AdamW
template <typename T>
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v, long n, float lr,
                             float b1, float b2, float eps, float wd, float bc1, float sbc2,
                             T* __restrict__ op, int* step_ctr, int step) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0 && step_ctr) step_ctr[0] = step;
  if (i >= n) return;
  const float gi = g[i];
  float pi = p[i] * (1.f - lr * wd);
  const float mi = b1 * m[i] + (1.f - b1) * gi;
  const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  pi -= (lr / bc1) * (mi / (sqrtf(vi) / sbc2 + eps));
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
  if (op) stf(op + i, pi);
}

// ---------------------------------------------------------------- noise injection
// Philox4x32-10 (Salmon et al., SC'11), all four output words
__device__ __forceinline__ void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                        uint32_t k0, uint32_t k1, uint32_t* o) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
// Box-Muller on 24-bit uniforms: u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float* z0, float* z1) {
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
  const float r = sqrtf(-2.f * logf(u1)), th = 6.283185307179586f * u2;
  *z0 = r * cosf(th);
  *z1 = r * sinf(th);
}

// one block per row: out = normalize(normalize(x) + sqrt(variance) n) (utils.py:19-31 with
// F.normalize's eps 1e-12), n for columns 4c .. 4c+3 from counter (row id, step, c, 0)
__global__ __launch_bounds__(256) void noise_inject_kernel(
    const float* x, int D, int ldx, const int* __restrict__ row_id,
    const int* __restrict__ step_ctr, uint32_t seed_lo, uint32_t seed_hi, float sd, float* out,
    int ldo) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  const float* xr = x + (long)r * ldx;
  float* orow = out + (long)r * ldo;
  const uint32_t rid = row_id ? (uint32_t)row_id[r] : (uint32_t)r;
  const uint32_t step = step_ctr ? (uint32_t)step_ctr[0] : 0u;
  float s = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) s = fmaf(xr[c], xr[c], s);
  const float inv = 1.f / fmaxf(sqrtf(block_sum(s, red)), 1e-12f);
  float q = 0.f;
  for (int c4 = threadIdx.x; 4 * c4 < D; c4 += 256) {
    uint32_t o[4];
    float z[4];
    philox4(rid, step, (uint32_t)c4, 0u, seed_lo, seed_hi, o);
    box_muller(o[0], o[1], &z[0], &z[1]);
    box_muller(o[2], o[3], &z[2], &z[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * c4 + e;
      if (c < D) {
        const float y = fmaf(sd, z[e], xr[c] * inv);
        orow[c] = y;
        q = fmaf(y, y, q);
      }
    }
  }
  const float inv2 = 1.f / fmaxf(sqrtf(block_sum(q, red)), 1e-12f);
  for (int c4 = threadIdx.x; 4 * c4 < D; c4 += 256)
    for (int e = 0; e < 4; ++e)
      if (4 * c4 + e < D) orow[4 * c4 + e] *= inv2;     // the thread's own values
}

__global__ void copy_rows_kernel(const float* __restrict__ x, int D, int ldx, float* __restrict__ out,
                                 int ldo) {
  const int r = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) out[(long)r * ldo + c] = x[(long)r * ldx + c];
}

}  // namespace tr
}  // namespace zs

using namespace zs;

#define ZS_DT(dtype, name) ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, name ": dtype")

extern "C" int zs_attention_bwd(const void* qkv, const void* d_out, int B, int L, const int* len,
                                int heads, void* dqkv, int dtype, void* stream) {
  ZS_REQUIRE(B > 0 && B <= 65535 && L >= 1 && L <= 256 && heads >= 1 && heads <= 1024,
             "zs_attention_bwd: 0 < B <= 65535, 1 <= L <= 256, 1 <= heads <= 1024");
  ZS_DT(dtype, "zs_attention_bwd");
  ZS_REQUIRE(qkv && d_out && dqkv, "zs_attention_bwd: null pointer");
  ZS_REQUIRE((((uintptr_t)qkv | (uintptr_t)d_out | (uintptr_t)dqkv) & 15) == 0,
             "zs_attention_bwd: qkv, d_out and dqkv 16-byte aligned");
  ZS_REQUIRE(qkv != dqkv && d_out != dqkv, "zs_attention_bwd: dqkv must not alias an input");
  const dim3 grid(heads, B);
  if (dtype == ZS_BF16)
    hipLaunchKernelGGL(tr::attention_bwd_kernel<bf16_t>, grid, dim3(256), 0, S(stream),
                       (const bf16_t*)qkv, (const bf16_t*)d_out, L, len, heads, (bf16_t*)dqkv);
  else
    hipLaunchKernelGGL(tr::attention_bwd_kernel<float>, grid, dim3(256), 0, S(stream),
                       (const float*)qkv, (const float*)d_out, L, len, heads, (float*)dqkv);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_layernorm_bwd(const float* x, int M, int C, int ldx, const int* rows,
                                const float* dy, int ldy, const float* g, float eps,
                                const float* res, int ldr, float* dx, int ldd, void* stream) {
  ZS_REQUIRE(M > 0 && C > 0 && ldx >= C && ldy >= C && ldd >= C && (!res || ldr >= C),
             "zs_layernorm_bwd: M, C > 0 and row strides >= C");
  ZS_REQUIRE(x && dy && dx, "zs_layernorm_bwd: null pointer");
  ZS_REQUIRE(eps >= 0.f, "zs_layernorm_bwd: eps >= 0");
  hipLaunchKernelGGL(tr::layernorm_bwd_kernel, dim3(cdiv(M, 4)), dim3(256), 0, S(stream), x, M, C,
                     ldx, rows, dy, ldy, g, eps, res, ldr, dx, ldd);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_gelu_tanh_bwd(const void* u, const float* dh, long n, void* du, int dtype,
                                void* stream) {
  ZS_REQUIRE(n > 0 && cdiv(n, 256) > 0, "zs_gelu_tanh_bwd: 0 < n < 2^39");
  ZS_DT(dtype, "zs_gelu_tanh_bwd");
  ZS_REQUIRE(u && dh && du, "zs_gelu_tanh_bwd: null pointer");
  if (dtype == ZS_BF16)
    hipLaunchKernelGGL(tr::gelu_tanh_bwd_kernel<bf16_t>, dim3(cdiv(n, 256)), dim3(256), 0, S(stream),
                       (const bf16_t*)u, dh, n, (bf16_t*)du);
  else
    hipLaunchKernelGGL(tr::gelu_tanh_bwd_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, S(stream),
                       (const float*)u, dh, n, (float*)du);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_tanh_bwd(const float* h, const float* dh, long n, float* dpre, void* stream) {
  ZS_REQUIRE(n > 0 && cdiv(n, 256) > 0, "zs_tanh_bwd: 0 < n < 2^39");
  ZS_REQUIRE(h && dh && dpre, "zs_tanh_bwd: null pointer");
  hipLaunchKernelGGL(tr::tanh_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, S(stream), h, dh, n, dpre);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_nll_grad_rows(const float* mix, int ldm, const void* wte, int V, int K,
                                const int* tgt, const int* cnt, int B, int M, float* dhf, int ldd,
                                int dtype, void* stream) {
  ZS_REQUIRE(M > 0 && B > 0 && V > 0 && K > 0 && ldm >= K && ldd >= K,
             "zs_nll_grad_rows: M, B, V, K > 0 and row strides >= K");
  ZS_DT(dtype, "zs_nll_grad_rows");
  ZS_REQUIRE(mix && wte && tgt && cnt && dhf, "zs_nll_grad_rows: null pointer");
  if (dtype == ZS_BF16)
    hipLaunchKernelGGL(tr::nll_grad_rows_kernel<bf16_t>, dim3(M), dim3(256), 0, S(stream), mix, ldm,
                       (const bf16_t*)wte, V, K, tgt, cnt, B, dhf, ldd);
  else
    hipLaunchKernelGGL(tr::nll_grad_rows_kernel<float>, dim3(M), dim3(256), 0, S(stream), mix, ldm,
                       (const float*)wte, V, K, tgt, cnt, B, dhf, ldd);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_nll_loss(const float* sum, const int* cnt, int B, float* loss, void* stream) {
  ZS_REQUIRE(B > 0, "zs_nll_loss: B > 0");
  ZS_REQUIRE(sum && cnt && loss, "zs_nll_loss: null pointer");
  hipLaunchKernelGGL(tr::nll_loss_kernel, dim3(1), dim3(64), 0, S(stream), sum, cnt, B, loss);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_soft_grad_rows(const float* dx, const int* hard_len, int h_cap, int n_soft, int B,
                                 int Smax, int D, float* d_soft, int ld, void* stream) {
  ZS_REQUIRE(B > 0 && B <= 65535 && n_soft >= 1 && h_cap >= 0 && D > 0 && Smax >= h_cap + n_soft &&
                 ld >= n_soft * D,
             "zs_soft_grad_rows: B, n_soft, D > 0, Smax >= h_cap + n_soft, ld >= n_soft * D");
  ZS_REQUIRE(dx && hard_len && d_soft, "zs_soft_grad_rows: null pointer");
  hipLaunchKernelGGL(tr::soft_grad_rows_kernel, dim3(n_soft, B), dim3(256), 0, S(stream), dx,
                     hard_len, h_cap, n_soft, Smax, D, d_soft, ld);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_colsum(const float* x, int B, int N, int ldx, float* out, void* stream) {
  ZS_REQUIRE(B > 0 && N > 0 && ldx >= N, "zs_colsum: B, N > 0, ldx >= N");
  ZS_REQUIRE(x && out, "zs_colsum: null pointer");
  hipLaunchKernelGGL(tr::colsum_kernel, dim3(cdiv(N, 256)), dim3(256), 0, S(stream), x, B, N, ldx, out);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_transpose_cast(const float* x, int R, int C, int ldx, void* y, int Rp, int dtype,
                                 void* stream) {
  ZS_REQUIRE(R > 0 && C > 0 && ldx >= C, "zs_transpose_cast: R, C > 0, ldx >= C");
  ZS_REQUIRE(Rp == (R + 31) / 32 * 32, "zs_transpose_cast: Rp = R rounded up to 32");
  ZS_REQUIRE(cdiv(Rp, 32) <= 65535, "zs_transpose_cast: R <= 65535 * 32");
  ZS_DT(dtype, "zs_transpose_cast");
  ZS_REQUIRE(x && y && (const void*)x != y, "zs_transpose_cast: null or aliased pointer");
  const dim3 grid(cdiv(C, 32), Rp / 32);
  if (dtype == ZS_BF16)
    hipLaunchKernelGGL(tr::transpose_cast_kernel<bf16_t>, grid, dim3(256), 0, S(stream), x, R, C,
                       ldx, (bf16_t*)y, Rp);
  else
    hipLaunchKernelGGL(tr::transpose_cast_kernel<float>, grid, dim3(256), 0, S(stream), x, R, C, ldx,
                       (float*)y, Rp);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int step, void* operand,
                        int dtype, int* step_ctr, void* stream) {
  ZS_REQUIRE(n > 0 && cdiv(n, 256) > 0, "zs_adamw: 0 < n < 2^39");
  ZS_REQUIRE(step >= 1, "zs_adamw: step >= 1 (the number of this update)");
  ZS_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f &&
                 weight_decay >= 0.f,
             "zs_adamw: 0 <= beta < 1, eps, lr, weight_decay >= 0");
  ZS_DT(dtype, "zs_adamw");
  ZS_REQUIRE(p && g && m && v, "zs_adamw: null pointer");
  // torch.optim.AdamW: bias_correction = 1 - beta^step (double, as Python computes them)
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float sbc2 = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  if (dtype == ZS_BF16)
    hipLaunchKernelGGL(tr::adamw_kernel<bf16_t>, dim3(cdiv(n, 256)), dim3(256), 0, S(stream), p, g, m,
                       v, n, lr, beta1, beta2, eps, weight_decay, bc1, sbc2, (bf16_t*)operand,
                       step_ctr, step);
  else
    hipLaunchKernelGGL(tr::adamw_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, S(stream), p, g, m,
                       v, n, lr, beta1, beta2, eps, weight_decay, bc1, sbc2, (float*)operand,
                       step_ctr, step);
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_noise_inject(const float* x, int B, int D, int ldx, const int* row_id,
                               const int* step_ctr, long seed, float variance, float* out, int ldo,
                               void* stream) {
  ZS_REQUIRE(B > 0 && D > 0 && ldx >= D && ldo >= D, "zs_noise_inject: B, D > 0, row strides >= D");
  ZS_REQUIRE(variance >= 0.f, "zs_noise_inject: variance >= 0");
  ZS_REQUIRE(x && out, "zs_noise_inject: null pointer");
  if (variance == 0.f) {
    if (x != out) {
      hipLaunchKernelGGL(tr::copy_rows_kernel, dim3(B), dim3(256), 0, S(stream), x, D, ldx, out, ldo);
      ZS_LAUNCH_CHECK();
    }
    return 0;
  }
  const uint64_t sd = (uint64_t)seed;
  hipLaunchKernelGGL(tr::noise_inject_kernel, dim3(B), dim3(256), 0, S(stream), x, D, ldx, row_id,
                     step_ctr, (uint32_t)sd, (uint32_t)(sd >> 32), sqrtf(variance), out, ldo);
  ZS_LAUNCH_CHECK();
  return 0;
}
