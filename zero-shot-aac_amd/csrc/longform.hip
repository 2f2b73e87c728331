// Long recordings: the back of a windowed pass.  A recording longer than the encoder's T samples
// is cut into overlapping windows (zs_resample_windows, frontend.hip); every window goes through
// the HTSAT pass and the tagging head like a clip of its own; zs_window_stitch puts the windows'
// outputs back onto one time line per recording:
//
//   timeline  the mean of the frame rows that cover a time-line frame (window w's frame j is
//             time-line frame w * hop_f + j), added in ascending w and divided by their count;
//   rec_clip  the maximum of the windows' clip probabilities (an event anywhere counts);
//   rec_emb   the windows' embeddings, weighted by each window's share of valid samples, summed
//             in ascending w and normalised as zs_l2norm_rows does.
//
// Pure memory traffic: every input element is read once, every output written once.  One wave
// per (time-line row, chunk of 256 columns) -- 16 bytes per lane where the leading dimensions
// allow it, one dword per lane otherwise -- taken from one work list over all recordings, so
// recordings of very different lengths share the grid evenly.  No atomics; an output is computed
// by one lane in a fixed order, so a recording's outputs do not depend on R or on its neighbours.
#include "common.h"

namespace zs {

constexpr int LF_FRAMES = 32;     // head frames per window
constexpr int LF_CHUNK = 256;     // columns per wave and work item

// the last r with plan[r].z (frow0) <= trow: frow0 ascends, a recording without frames shares
// its frow0 with the next one, which is the one found
__device__ __forceinline__ int lf_find(const int4* __restrict__ plan, int R, int trow) {
  int lo = 0, hi = R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (plan[mid].z <= trow) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <bool VEC>
__global__ __launch_bounds__(256) void stitch_timeline_kernel(
    const int4* __restrict__ plan, int R, int hop_f, int N, const float* __restrict__ frame,
    int ldf, float* __restrict__ timeline, int ldt) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nchunk = cdiv(N, LF_CHUNK);
  const int4 last = plan[R - 1];
  const long total = (long)(last.z + last.w) * nchunk;
  for (long it = (long)blockIdx.x * 4 + wid; it < total; it += (long)gridDim.x * 4) {
    const int trow = (int)(it / nchunk), c0 = (int)(it % nchunk) * LF_CHUNK;
    const int4 p = plan[lf_find(plan, R, trow)];      // (row0, n_win, frow0, F)
    const int f = trow - p.z;
    // windows w with 0 <= f - w * hop_f < 32
    const int w_lo = f < LF_FRAMES ? 0 : (f - LF_FRAMES + hop_f) / hop_f;
    const int w_hi = min(p.y - 1, f / hop_f);
    const int cnt = w_hi - w_lo + 1;
    const float* src = frame + ((long)(p.x + w_lo) * LF_FRAMES + (f - w_lo * hop_f)) * ldf;
    const long wstep = (long)(LF_FRAMES - hop_f) * ldf;    // window w + 1, the same time-line frame
    float* dst = timeline + (long)trow * ldt;
    if (VEC) {
      const int c = c0 + 4 * lane;
      if (c + 4 <= N) {
        float4 s = *reinterpret_cast<const float4*>(src + c);
        for (int w = 1; w < cnt; ++w) {
          const float4 v = *reinterpret_cast<const float4*>(src + w * wstep + c);
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (cnt > 1) {
          const float d = (float)cnt;
          s = make_float4(__fdiv_rn(s.x, d), __fdiv_rn(s.y, d), __fdiv_rn(s.z, d), __fdiv_rn(s.w, d));
        }
        *reinterpret_cast<float4*>(dst + c) = s;
      } else {
        for (int k = c; k < N; ++k) {                 // the row's last, partial quad
          float s = src[k];
          for (int w = 1; w < cnt; ++w) s += src[w * wstep + k];
          dst[k] = cnt > 1 ? __fdiv_rn(s, (float)cnt) : s;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < LF_CHUNK / 64; ++q) {
        const int k = c0 + 64 * q + lane;
        if (k >= N) break;
        float s = src[k];
        for (int w = 1; w < cnt; ++w) s += src[w * wstep + k];
        dst[k] = cnt > 1 ? __fdiv_rn(s, (float)cnt) : s;
      }
    }
  }
}

// rec_clip[r][k] = max_w clip[row0 + w][k] for k < N, -inf for N <= k < ldrc
__global__ __launch_bounds__(256) void stitch_clip_kernel(
    const int4* __restrict__ plan, int R, int N, const float* __restrict__ clip, int ldc,
    float* __restrict__ rec_clip, int ldrc) {
  const int nchunk = cdiv(ldrc, 256);
  const long total = (long)R * nchunk;
  for (long it = blockIdx.x; it < total; it += gridDim.x) {
    const int r = (int)(it / nchunk), k = (int)(it % nchunk) * 256 + threadIdx.x;
    if (k >= ldrc) continue;
    const int4 p = plan[r];
    float m = -INFINITY;
    if (k < N) {
      const float* src = clip + (long)p.x * ldc + k;
      for (int w = 0; w < p.y; ++w) m = fmaxf(m, src[(long)w * ldc]);
    }
    rec_clip[(long)r * ldrc + k] = m;
  }
}

// rec_emb[r] = s / max(||s||, 1e-12), s = sum_w wgt[row0 + w] * emb[row0 + w]; one wave per
// recording, K / 64 columns per lane in registers (K <= 2048); n_win == 1 copies the row
__global__ __launch_bounds__(256) void stitch_emb_kernel(
    const int4* __restrict__ plan, const float* __restrict__ wgt, int R, int K,
    const float* __restrict__ emb, int lde, float* __restrict__ rec_emb, int ldre) {
  constexpr int Q = 2048 / 64;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int4 p = plan[r];
  const float* src = emb + (long)p.x * lde;
  float* dst = rec_emb + (long)r * ldre;
  if (p.y == 1) {
    for (int c = lane; c < K; c += 64) dst[c] = src[c];
    return;
  }
  float s[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) s[q] = 0.f;
  for (int w = 0; w < p.y; ++w) {
    const float g = wgt[p.x + w];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int c = lane + 64 * q;
      if (c < K) s[q] = __fadd_rn(s[q], __fmul_rn(g, src[(long)w * lde + c]));
    }
  }
  float ss = 0.f;                           // zs_l2norm_rows' order: per lane by column, then the wave
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (lane + 64 * q < K) ss += s[q] * s[q];
  const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = lane + 64 * q;
    if (c < K) dst[c] = s[q] * inv;
  }
}

}  // namespace zs

using namespace zs;

extern "C" int zs_window_stitch(const int* plan, const float* wgt, int R, int hop_f, int N,
                                const float* frame, int ldf, const float* clip, int ldc,
                                const float* emb, int lde, int K, float* timeline, int ldt,
                                float* rec_clip, int ldrc, float* rec_emb, int ldre,
                                void* stream) {
  ZS_REQUIRE(plan && wgt, "zs_window_stitch: NULL plan / wgt");
  ZS_REQUIRE(((uintptr_t)plan & 15) == 0, "zs_window_stitch: plan 16-byte aligned");
  ZS_REQUIRE(R > 0, "zs_window_stitch: R > 0");
  ZS_REQUIRE(hop_f >= 1 && hop_f <= LF_FRAMES, "zs_window_stitch: hop_f %d outside [1, 32]", hop_f);
  ZS_REQUIRE(N > 0, "zs_window_stitch: N > 0");
  ZS_REQUIRE(timeline || rec_clip || rec_emb, "zs_window_stitch: no output given");
  ZS_REQUIRE(!timeline || frame, "zs_window_stitch: timeline given without frame");
  ZS_REQUIRE(!rec_clip || clip, "zs_window_stitch: rec_clip given without clip");
  ZS_REQUIRE(!rec_emb || emb, "zs_window_stitch: rec_emb given without emb");
  ZS_REQUIRE(!timeline || (ldf >= N && ldt >= N), "zs_window_stitch: ldf %d / ldt %d < N %d", ldf, ldt, N);
  ZS_REQUIRE(!rec_clip || (ldc >= N && ldrc >= N), "zs_window_stitch: ldc %d / ldrc %d < N %d", ldc, ldrc, N);
  ZS_REQUIRE(!rec_emb || (K > 0 && K % 32 == 0 && K <= 2048),
             "zs_window_stitch: K %d (a multiple of 32, at most 2048)", K);
  ZS_REQUIRE(!rec_emb || (lde >= K && ldre >= K), "zs_window_stitch: lde %d / ldre %d < K %d", lde, ldre, K);
  const int4* pl = reinterpret_cast<const int4*>(plan);
  if (timeline) {
    const bool vec = ldf % 4 == 0 && ldt % 4 == 0 && (((uintptr_t)frame | (uintptr_t)timeline) & 15) == 0;
    const dim3 grid(256 * 8);               // 4 waves each, striding over the work list
    if (vec)
      hipLaunchKernelGGL(stitch_timeline_kernel<true>, grid, dim3(256), 0, S(stream), pl, R, hop_f, N,
                         frame, ldf, timeline, ldt);
    else
      hipLaunchKernelGGL(stitch_timeline_kernel<false>, grid, dim3(256), 0, S(stream), pl, R, hop_f, N,
                         frame, ldf, timeline, ldt);
    ZS_LAUNCH_CHECK();
  }
  if (rec_clip) {
    const long items = (long)R * cdiv(ldrc, 256);
    hipLaunchKernelGGL(stitch_clip_kernel, dim3((unsigned)std::min(items, 256L * 8)), dim3(256), 0,
                       S(stream), pl, R, N, clip, ldc, rec_clip, ldrc);
    ZS_LAUNCH_CHECK();
  }
  if (rec_emb) {
    hipLaunchKernelGGL(stitch_emb_kernel, dim3(cdiv(R, 4)), dim3(256), 0, S(stream), pl, wgt, R, K,
                       emb, lde, rec_emb, ldre);
    ZS_LAUNCH_CHECK();
  }
  return 0;
}
