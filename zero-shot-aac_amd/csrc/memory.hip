// Projection of embeddings onto a memory bank (map2memory, predict_prompt.py:23-29):
//   z[m][n] = scale * (Q[m] . B[n]),  w = softmax_n(z),  mix[m] = sum_n w[m][n] B[n]
// as ONE streaming pass over the bank -- a flash-decoding pass with K = V = the bank, one head and
// head dim K <= 1024 -- and a merge kernel.  No [M][N] array exists anywhere.  DESIGN.md §27.
//
// memory_project_kernel: a workgroup of 8 waves owns 32 query rows and one split of the bank rows
// and walks the split in tiles of BN rows (32 bf16 / 16 f32).  The K columns are cut into units
// of 32; wave w owns units w*UPW .. w*UPW + UPW - 1 for BOTH products, so its slice of the 32 x K
// accumulator (16 registers per unit) and its slice of Q (as MFMA operands) stay in registers for
// the whole pass.  Per tile:
//   stage    the tile's rows go global -> registers (issued one tile ahead) -> LDS, whole rows,
//            coalesced; rows past the split's end are zeros.  This LDS image serves both products.
//   phase 1  every wave multiplies its column slice: a partial S [32][BN] -> LDS, one per wave
//   softmax  wave w adds the 8 partials of rows 4w .. 4w+3 in wave order, times scale, and runs
//            the online softmax of those rows (running max m, running sum l; lanes 16g .. 16g+15
//            hold one row); P (bf16-rounded for bf16 banks, and l adds the rounded values) and
//            the rows' rescale factors exp(m_old - m_new) go to LDS
//   phase 2  every wave rescales its accumulator slice and adds P . tile[:, its columns]: bf16
//            reads the row-major image column-wise with ds_read_b64_tr_b16, f32 with plain
//            32-bit reads (v_mfma_f32_32x32x2_f32 takes one k per lane half)
// Each split writes (a [K], m, l) per row; memory_merge_kernel combines them in split order.
// Nothing is atomic and no reduction order depends on M, so a row's result is the same whatever
// shares the launch, and the same from run to run.
#include "common.h"
#include "gemm_core.h"

namespace zs {
namespace mem {

constexpr int BM = 32;            // query rows per workgroup
constexpr int NW = 8;             // waves per workgroup
constexpr int NT = 64 * NW;
constexpr int MAX_NSPLIT = 4096;  // the merge kernel keeps one weight per split in LDS
constexpr int PSTRIDE = 80;       // bytes per row of the P image (64 B of data; 80 = 5 x 16:
                                  // the 16-byte row reads of 16 rows fall on 16 distinct slots)

template <typename T> struct Tile;
template <> struct Tile<bf16_t> { static constexpr int BN = 32, WANT = 80; };
template <> struct Tile<float> { static constexpr int BN = 16, WANT = 16; };

// bytes per LDS row of a bank tile: the K values plus a pad that makes the stride = WANT (mod
// 256), a multiple of 16.  bf16, 80: the 16-byte row reads of phase 1 (one row per lane) are
// conflict-free (80 / 16 = 5 is odd) and the four rows of a transposed read land 20 banks apart.
// f32, 16: the row reads of phase 1 are conflict-free; phase 2 reads whole rows.
template <typename T> __host__ __device__ inline int tile_stride(int K) {
  const int rb = K * (int)sizeof(T);
  return rb + ((Tile<T>::WANT - rb) & 255);
}
template <typename T> __host__ __device__ inline int lds_bytes(int K) {
  constexpr int BN = Tile<T>::BN;
  return BN * tile_stride<T>(K) + NW * BM * BN * 4 + BM * PSTRIDE + BM * 4;
}

// all-reduce over a row of 16 lanes with DPP row rotations (one VALU op each; __shfl_xor goes
// through ds_bpermute and costs an LDS round trip per step).  Every lane ends with the max; the
// sum's association differs from lane to lane, so only one fixed lane's sum may be used.
template <int CTRL> __device__ __forceinline__ float dpp_row(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_row<0x128>(v));   // row_ror:8
  v = fmaxf(v, dpp_row<0x124>(v));   // row_ror:4
  v = fmaxf(v, dpp_row<0x122>(v));   // row_ror:2
  return fmaxf(v, dpp_row<0x121>(v));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_row<0x128>(v);
  v += dpp_row<0x124>(v);
  v += dpp_row<0x122>(v);
  return v + dpp_row<0x121>(v);
}

typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

template <typename T, int UPW>
__global__ __launch_bounds__(NT) void memory_project_kernel(int M, int N, int K, const T* __restrict__ Q,
                                                            int ldq, const T* __restrict__ B, int ldb,
                                                            float scale, int nsplit, int rows_per,
                                                            float* __restrict__ part_mix,
                                                            float* __restrict__ part_ml) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int BN = Tile<T>::BN;
  constexpr int EPL = BN / 16;            // S elements per lane in the softmax stage
  // staging passes per thread: BN * cprp / NT with cprp <= 32 UPW rounded up to a power of two
  constexpr int NCH = UPW == 3 ? 8 : 2 * UPW;
  constexpr int VPC = 16 / (int)sizeof(T);  // values per chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int stride = tile_stride<T>(K);
  char* tile = smem;
  float* spart = reinterpret_cast<float*>(smem + BN * stride);          // [NW][BM][BN]
  char* pimg = reinterpret_cast<char*>(spart + NW * BM * BN);           // [BM] rows of PSTRIDE
  float* alpha_s = reinterpret_cast<float*>(pimg + BM * PSTRIDE);       // [BM]

  // the wave index in a scalar register: every test of a unit's validity is a scalar branch
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int split = blockIdx.x % nsplit, m0 = (blockIdx.x / nsplit) * BM;
  const int nu = K >> 5;
  const long nb = (long)split * rows_per;
  const int n_beg = nb < N ? (int)nb : N;
  const int n_end = nb + rows_per < N ? (int)(nb + rows_per) : N;

  // this wave's slice of Q as MFMA operands, zeros for rows past M
  bf16x8_t qb[UPW][2];
  float qf[UPW][16];
  f32x16_t acc[UPW];
#pragma unroll
  for (int i = 0; i < UPW; ++i) {
    const int u = w * UPW + i;
    const bool ok = u < nu && m0 + r < M;
    const T* qrow = Q + (long)(m0 + r) * ldq + u * 32;
    if constexpr (BF) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = *reinterpret_cast<const uint4*>(qrow + s * 16 + h * 8);
        qb[i][s] = __builtin_bit_cast(bf16x8_t, v);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) v = *reinterpret_cast<const float4*>(qrow + h * 16 + j * 4);
        qf[i][4 * j + 0] = v.x; qf[i][4 * j + 1] = v.y; qf[i][4 * j + 2] = v.z; qf[i][4 * j + 3] = v.w;
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  }
  // softmax stage: lanes 16g .. 16g+15 of wave w hold row 4w + g
  const int srow = 4 * w + (lane >> 4), l16 = lane & 15;
  float run_m = -INFINITY, run_l = 0.f;

  // staging: a row's 16-byte chunks sit on cprp consecutive threads (cprp = the chunks per row
  // rounded up to a power of two), NT / cprp rows per pass, so pass c of a thread is its first
  // address plus c times a uniform step, in global memory and in LDS
  const int cpr = (K * (int)sizeof(T)) >> 4;
  int csh = 2;
  while ((1 << csh) < cpr) ++csh;
  const int ch = tid & ((1 << csh) - 1), row0 = tid >> csh, rpp = NT >> csh;
  const bool ch_ok = ch < cpr;
  // every pass loads unconditionally from a row clamped into the split (and chunk 0 for the idle
  // threads of a K that is no power of two): no branch sits between a load and its use, so the
  // loads of the next tile stay in flight across both products.  What lies past the split's end
  // becomes zeros when the registers go to LDS.
  const T* gsrc = B + (ch_ok ? ch : 0) * VPC;
  char* ldst = tile + row0 * stride + ch * 16;
  uint4 pre[NCH];
  auto fetch = [&](int n0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int n = n0 + row0 + c * rpp;
      pre[c] = *reinterpret_cast<const uint4*>(gsrc + (long)(n < n_end ? n : n_end - 1) * ldb);
    }
  };
  // Q has arrived before the first tile is asked for: from here on the only loads in flight are
  // a tile's, and no wait in the loop has to cover anything older
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), the other counters untouched
  if (n_beg < n_end) fetch(n_beg);

  for (int n0 = n_beg; n0 < n_end; n0 += BN) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int row = row0 + c * rpp;
      if (ch_ok && row < BN)
        *reinterpret_cast<uint4*>(ldst + c * rpp * stride) = n0 + row < n_end ? pre[c] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    // the next tile's loads: bf16 before phase 1; f32 before phase 2, where its 64 Q registers
    // and the S tile no longer compete with the 32 staging registers (no spill at K = 1024)
    if (BF && n0 + BN < n_end) fetch(n0 + BN);

    // ---- phase 1: S[m][n] over this wave's columns (A = Q, B = the tile's rows)
    {
      f32x16_t s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
      for (int i = 0; i < UPW; ++i) {
        const int u = w * UPW + i;
        if (u < nu) {
          if constexpr (BF) {
            const char* p = tile + r * stride + (u * 32 + h * 8) * 2;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(p + s2 * 32);
              s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qb[i][s2], b, s, 0, 0, 0);
            }
          } else {
            // columns 16 .. 31 of S repeat 0 .. 15 (BN = 16) and are not stored
            const float* p = reinterpret_cast<const float*>(tile + (r & 15) * stride) + u * 32 + h * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float4 b = *reinterpret_cast<const float4*>(p + 4 * j);
              s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i][4 * j + 0], b.x, s, 0, 0, 0);
              s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i][4 * j + 1], b.y, s, 0, 0, 0);
              s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i][4 * j + 2], b.z, s, 0, 0, 0);
              s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i][4 * j + 3], b.w, s, 0, 0, 0);
            }
            // keep the next unit's 16 operand registers from being loaded a unit early (with
            // 64 registers of Q and 64 of accumulators that is what spills at K = 1024)
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      if (r < BN) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          spart[(w * BM + (e & 3) + 8 * (e >> 2) + 4 * h) * BN + r] = s[e];
      }
    }
    __syncthreads();

    // ---- online softmax of rows 4w .. 4w+3
    {
      float z[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) z[e] = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww)
#pragma unroll
        for (int e = 0; e < EPL; ++e) z[e] += spart[(ww * BM + srow) * BN + l16 * EPL + e];
      float tmax = -INFINITY;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        z[e] = n0 + l16 * EPL + e < n_end ? scale * z[e] : -INFINITY;
        tmax = fmaxf(tmax, z[e]);
      }
      tmax = row16_max(tmax);
      const float m_new = fmaxf(run_m, tmax);
      const float alpha = run_m == -INFINITY ? 0.f : expf(run_m - m_new);
      float psum = 0.f;
      float p[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        p[e] = z[e] == -INFINITY ? 0.f : expf(z[e] - m_new);
        if constexpr (BF) p[e] = bf2f(f2bf(p[e]));
        psum += p[e];
      }
      // (only lane 16g of a row's lanes writes l at the end: see row16_sum)
      run_l = run_l * alpha + row16_sum(psum);
      run_m = m_new;
      if constexpr (BF)
        *reinterpret_cast<uint32_t*>(pimg + srow * PSTRIDE + l16 * 4) = pk2bf(p[0], p[1]);
      else
        *reinterpret_cast<float*>(pimg + srow * PSTRIDE + l16 * 4) = p[0];
      if (l16 == 0) alpha_s[srow] = alpha;
    }
    __syncthreads();

    // ---- phase 2: acc[m][c] = alpha[m] acc[m][c] + sum_n P[m][n] tile[n][c]
    if (!BF && n0 + BN < n_end) fetch(n0 + BN);
    {
      float al[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(alpha_s + 8 * g + 4 * h);
        al[4 * g + 0] = a.x; al[4 * g + 1] = a.y; al[4 * g + 2] = a.z; al[4 * g + 3] = a.w;
      }
      if constexpr (BF) {
        bf16x8_t pa[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          pa[s2] = *reinterpret_cast<const bf16x8_t*>(pimg + r * PSTRIDE + (s2 * 16 + h * 8) * 2);
        // transposed read: lane 4q+p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a
        // 4 x 16 block and receives the block's column (lane & 15), rows 0 .. 3.  Lane (r, h)
        // wants tile[16 s2 + 8h + j][u*32 + r], j = 0 .. 7: two blocks, rows 8h + 4t .. + 3
        const int q = (lane & 15) >> 2, pcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
        const char* tb = tile + (8 * h + q) * stride + pcol * 2;
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
          const int u = w * UPW + i;
          if (u < nu) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] *= al[e];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const char* a0 = tb + (16 * s2) * stride + u * 64;
              const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                  (__attribute__((address_space(3))) s16x4_t*)(a0));
              const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                  (__attribute__((address_space(3))) s16x4_t*)(a0 + 4 * stride));
              const s16x8_t b8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[s2], __builtin_bit_cast(bf16x8_t, b8),
                                                               acc[i], 0, 0, 0);
            }
          }
        }
      } else {
        float pf[8];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float4 a = *reinterpret_cast<const float4*>(pimg + r * PSTRIDE + (8 * h + 4 * j) * 4);
          pf[4 * j + 0] = a.x; pf[4 * j + 1] = a.y; pf[4 * j + 2] = a.z; pf[4 * j + 3] = a.w;
        }
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
          const int u = w * UPW + i;
          if (u < nu) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] *= al[e];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float b = *(reinterpret_cast<const float*>(tile + (8 * h + j) * stride) + u * 32 + r);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf[j], b, acc[i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    __syncthreads();
  }

  // the split's partial: a [K], (m, l) per row; an empty split leaves (0, -inf, 0).  The lane
  // coordinates are derived again behind an opaque copy of the thread index, so no output address
  // is computed ahead of the loop and carried through it in registers the loop needs
  int t2 = tid;
  asm volatile("" : "+v"(t2));
  const int w2 = t2 >> 6, r2 = t2 & 31, h2 = (t2 >> 5) & 1;
#pragma unroll
  for (int i = 0; i < UPW; ++i) {
    const int u = w2 * UPW + i;
    if (u < nu) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + (e & 3) + 8 * (e >> 2) + 4 * h2;
        if (m < M) part_mix[((long)m * nsplit + split) * K + u * 32 + r2] = acc[i][e];
      }
    }
  }
  const int srow2 = 4 * w2 + ((t2 >> 4) & 3);
  if ((t2 & 15) == 0 && m0 + srow2 < M) {
    float* ml = part_ml + ((long)(m0 + srow2) * nsplit + split) * 2;
    ml[0] = run_m;
    ml[1] = run_l;
  }
}

// One workgroup per row: m* = max m_s, weight_s = exp(m_s - m*) (0 for an empty split),
// L = sum l_s weight_s and mix = sum a_s weight_s / L, both added in split order by every thread
// that needs them; then the optional L2 normalisation (eps convention of zs_l2norm_rows).
__global__ __launch_bounds__(256) void memory_merge_kernel(const float* __restrict__ part_mix,
                                                           const float* __restrict__ part_ml, int nsplit,
                                                           int K, int normalize, float* __restrict__ out,
                                                           int ldo, float* __restrict__ lse) {
  extern __shared__ float wts[];   // [nsplit] weights, then [4] for block_sum
  float* red = wts + nsplit;
  const int m = blockIdx.x;
  const float* ml = part_ml + (long)m * nsplit * 2;
  float mx = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, ml[2 * s]);
  for (int s = threadIdx.x; s < nsplit; s += 256) {
    const float ms = ml[2 * s];
    wts[s] = ms == -INFINITY ? 0.f : expf(ms - mx);
  }
  __syncthreads();
  float L = 0.f;
  for (int s = 0; s < nsplit; ++s) L += ml[2 * s + 1] * wts[s];
  float v[4];
  float ssq = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = threadIdx.x + 256 * j;
    v[j] = 0.f;
    if (c < K) {
      const float* a = part_mix + (long)m * nsplit * K + c;
      float t = 0.f;
      // an empty split's a is zeros by contract, so no test sits between the loads
#pragma unroll 8
      for (int s = 0; s < nsplit; ++s) t += a[(long)s * K] * wts[s];
      v[j] = L > 0.f ? t / L : 0.f;   // a true division: exact sums give the exact mean
      ssq += v[j] * v[j];
    }
  }
  float sc = 1.0f;
  if (normalize) sc = 1.0f / fmaxf(sqrtf(block_sum(ssq, red)), 1e-12f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = threadIdx.x + 256 * j;
    if (c < K) out[(long)m * ldo + c] = v[j] * sc;
  }
  if (lse != nullptr && threadIdx.x == 0) lse[m] = L > 0.f ? mx + logf(L) : -INFINITY;
}

template <typename T, int UPW>
static int launch_project(int M, int N, int K, const void* Q, int ldq, const void* B, int ldb,
                          float scale, int nsplit, float* part_mix, float* part_ml, hipStream_t st) {
  constexpr int BN = Tile<T>::BN;
  const int rows_per = cdiv(cdiv(N, nsplit), BN) * BN;
  const int lds = lds_bytes<T>(K);
  static bool attr = false;   // per instantiation: more than 64 KiB of dynamic LDS
  if (!attr) {
    ZS_CHECK_HIP(hipFuncSetAttribute((const void*)memory_project_kernel<T, UPW>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes<T>(256 * UPW)));
    attr = true;
  }
  hipLaunchKernelGGL((memory_project_kernel<T, UPW>), dim3((unsigned)(nsplit * cdiv(M, BM))), dim3(NT),
                     lds, st, M, N, K, (const T*)Q, ldq, (const T*)B, ldb, scale, nsplit, rows_per,
                     part_mix, part_ml);
  ZS_LAUNCH_CHECK();
  return ZS_OK;
}

template <typename T>
static int dispatch_project(int M, int N, int K, const void* Q, int ldq, const void* B, int ldb,
                            float scale, int nsplit, float* part_mix, float* part_ml, hipStream_t st) {
  const int upw = cdiv(K >> 5, NW);
  switch (upw) {
    case 1: return launch_project<T, 1>(M, N, K, Q, ldq, B, ldb, scale, nsplit, part_mix, part_ml, st);
    case 2: return launch_project<T, 2>(M, N, K, Q, ldq, B, ldb, scale, nsplit, part_mix, part_ml, st);
    case 3: return launch_project<T, 3>(M, N, K, Q, ldq, B, ldb, scale, nsplit, part_mix, part_ml, st);
    default: return launch_project<T, 4>(M, N, K, Q, ldq, B, ldb, scale, nsplit, part_mix, part_ml, st);
  }
}

}  // namespace mem
}  // namespace zs

using namespace zs;

extern "C" int zs_memory_nsplit(int N, int K, int dtype) {
  ZS_REQUIRE(N > 0 && K % 32 == 0 && K >= 32 && K <= 1024, "zs_memory_nsplit: N > 0, K %% 32, 32 <= K <= 1024");
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "zs_memory_nsplit: dtype");
  // at least 512 bank rows per split, at most 128 splits: two row blocks of 128 splits fill the
  // 256 CUs once, and a multiple of 8 keeps the row blocks of one split on one XCD
  const int s = cdiv(N, 512);
  return s < 1 ? 1 : s > 128 ? 128 : s;
}

extern "C" int zs_memory_project(int M, int N, int K, int dtype, const void* Q, int ldq,
                                 const void* bank, int ldb, float scale, int nsplit, float* part_mix,
                                 float* part_ml, void* stream) {
  ZS_REQUIRE(M > 0 && N > 0 && N <= 0x7fffffff - 1024, "zs_memory_project: M, N > 0 (N < 2^31 - 1024)");
  ZS_REQUIRE(K % 32 == 0 && K >= 32 && K <= 1024, "zs_memory_project: K %% 32 and 32 <= K <= 1024");
  ZS_REQUIRE(ldq % 8 == 0 && ldb % 8 == 0 && ldq >= K && ldb >= K,
             "zs_memory_project: ldq / ldb %% 8 and >= K");
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "zs_memory_project: dtype");
  ZS_REQUIRE(nsplit >= 1 && nsplit <= mem::MAX_NSPLIT, "zs_memory_project: 1 <= nsplit <= %d",
             mem::MAX_NSPLIT);
  ZS_REQUIRE(Q && bank && part_mix && part_ml, "zs_memory_project: null pointer");
  ZS_REQUIRE((((uintptr_t)Q | (uintptr_t)bank | (uintptr_t)part_mix) & 15) == 0 &&
                 ((uintptr_t)part_ml & 7) == 0,
             "zs_memory_project: Q, bank and part_mix must be 16-byte aligned");
  ZS_REQUIRE((long)nsplit * cdiv(M, mem::BM) < (1L << 31), "zs_memory_project: the grid does not fit an int");
  hipStream_t st = S(stream);
  if (dtype == ZS_BF16)
    return mem::dispatch_project<bf16_t>(M, N, K, Q, ldq, bank, ldb, scale, nsplit, part_mix, part_ml, st);
  return mem::dispatch_project<float>(M, N, K, Q, ldq, bank, ldb, scale, nsplit, part_mix, part_ml, st);
}

extern "C" int zs_memory_merge(const float* part_mix, const float* part_ml, int M, int nsplit, int K,
                               int normalize, float* out, int ldo, float* lse, void* stream) {
  ZS_REQUIRE(M > 0 && nsplit >= 1 && nsplit <= mem::MAX_NSPLIT, "zs_memory_merge: M > 0, 1 <= nsplit <= %d",
             mem::MAX_NSPLIT);
  ZS_REQUIRE(K % 32 == 0 && K >= 32 && K <= 1024, "zs_memory_merge: K %% 32 and 32 <= K <= 1024");
  ZS_REQUIRE(ldo % 8 == 0 && ldo >= K, "zs_memory_merge: ldo %% 8 and >= K");
  ZS_REQUIRE(part_mix && part_ml && out, "zs_memory_merge: null pointer");
  ZS_REQUIRE((((uintptr_t)part_mix | (uintptr_t)out) & 15) == 0 && ((uintptr_t)part_ml & 7) == 0,
             "zs_memory_merge: part_mix and out must be 16-byte aligned");
  hipLaunchKernelGGL(mem::memory_merge_kernel, dim3((unsigned)M), dim3(256), (nsplit + 4) * sizeof(float),
                     S(stream), part_mix, part_ml, nsplit, K, normalize, out, ldo, lse);
  ZS_LAUNCH_CHECK();
  return ZS_OK;
}
