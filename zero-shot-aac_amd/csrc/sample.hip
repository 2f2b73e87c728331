// Sampling one token per row from f32 logits (generate2's top_p / temperature arguments,
// gpt2_prefix_eval.py:161-222, with the nucleus rule of its lines 197-206; HF's processor order:
// temperature, top-k, top-p), without a sort.  DESIGN.md §28.
//
// sample_rows_kernel: ONE workgroup of 16 waves per row, the row in registers (NV4 float4 per
// lane, 1024 x 4 NV4 >= V values, read once).  Wave w owns the ids [w 256 NV4, (w + 1) 256 NV4);
// float4 j of lane l holds the ids w 256 NV4 + (64 j + l) 4 .. + 3 -- every load is one coalesced
// 1 KiB per wave, and the id order inside a wave is (j, lane, element).
//   stats    max and sum exp(x - max) of the raw logits (the log-probability reported is the
//            temperature-1, unfiltered one) and sum exp(z - max z) of z = x / temperature
//   top-k    the k-th largest z by bisection, bit by bit, on the order-preserving integer image
//            of the float (f2key): 32 block counts; the ties at the cut are admitted by id
//            (a second bisection, on the id, over the count of ties below it)
//   p        registers become exp(z - max z) for what is kept, -1 for what is not
//   top-p    the nucleus boundary by the same bisection on the bits of p (p >= 0: the bits are
//            order-preserving): the largest t with sum_{p >= t} p > top_p S; everything above t
//            is kept, and of the n ties at t the first m by id, m = #{q < n: G + q t <= top_p S},
//            G = sum_{p > t} p (rank 0 is always kept: G <= top_p S by the choice of t)
//   draw     an id-order prefix sum: per wave NV4 lane scans with a carry, the 16 wave totals
//            added in wave order; the token is the lowest kept id whose running mass exceeds
//            u M (the last kept id if rounding leaves none)
// Every reduction is a wave butterfly plus 16 partials added in wave order by every thread, and
// counts are integers: nothing is atomic, nothing depends on R or on the row's slot in the
// launch, and the same inputs give the same bits on every run.
#include "common.h"

namespace zs {
namespace smp {

constexpr int NT = 1024;
constexpr int NW = NT / 64;
constexpr int MAX_V = NT * 64;

// The loops over a lane's 64 values end each float4 with a scheduling fence.  Without it the
// scheduler interleaves all 16 float4 of a pass (64 compare masks in scalar registers, 64
// exponentials in flight) beside the 64 values that have to stay in registers, and spills.
#define ZS_ONE_AT_A_TIME() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
  return v;
}

// Block reductions with ONE barrier each: the partials alternate between two LDS rows, and a
// thread that writes a row again has passed the barrier of the reduction in between, which every
// thread reaches only after it has read that row.
struct Block {
  uint32_t* red;   // [2][NW]
  int par, lane, wid;
  __device__ __forceinline__ uint32_t* put(uint32_t w) {
    uint32_t* b = red + par * NW;
    par ^= 1;
    if (lane == 0) b[wid] = w;
    __syncthreads();
    return b;
  }
  __device__ __forceinline__ float sum(float v) {
    const uint32_t* b = put(__float_as_uint(wave_sum(v)));
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) t += __uint_as_float(b[i]);
    return t;
  }
  __device__ __forceinline__ float max(float v) {
    const uint32_t* b = put(__float_as_uint(wave_max(v)));
    float t = -INFINITY;
#pragma unroll
    for (int i = 0; i < NW; ++i) t = fmaxf(t, __uint_as_float(b[i]));
    return t;
  }
  __device__ __forceinline__ unsigned sum_u(unsigned v) {
    const uint32_t* b = put(wave_sum_u(v));
    unsigned t = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) t += b[i];
    return t;
  }
  __device__ __forceinline__ unsigned min_u(unsigned v) {
    const uint32_t* b = put(wave_min_u(v));
    unsigned t = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < NW; ++i) t = ::min(t, b[i]);
    return t;
  }
  __device__ __forceinline__ unsigned max_u(unsigned v) {
    const uint32_t* b = put(wave_max_u(v));
    unsigned t = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) t = ::max(t, b[i]);
    return t;
  }
};

// Philox4x32-10 (Salmon et al., SC'11), first output word
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ float wave_incl_scan(float x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(x, o, 64);
    if (lane >= o) x += t;
  }
  return x;
}

template <int NV4>
__global__ __launch_bounds__(NT) void sample_rows_kernel(
    const float* __restrict__ logits, int V, int ld, int vec, const int* __restrict__ row_id,
    const int* step_ctr, uint32_t seed_lo, uint32_t seed_hi, float temperature, int top_k,
    float top_p, float* __restrict__ part_val, int* __restrict__ part_idx,
    float* __restrict__ logprob, float* __restrict__ kept) {
  __shared__ uint32_t red[2 * NW];
  __shared__ float wtot[NW];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  Block blk{red, 0, lane, wid};
  const float* row = logits + (long)r * ld;
  const int id_l = wid * (256 * NV4) + lane * 4;   // id of (j, e) = id_l + 256 j + e
  // an opaque copy per use: the 64 ids are then recomputed inside each loop (one add each), not
  // computed once and carried in 64 registers next to the 64 values
  auto ids = [&]() -> int {
    int t = id_l;
    asm volatile("" : "+v"(t));
    return t;
  };

  // ---- the row: raw logits first, for the temperature-1 statistics
  float v[NV4][4];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV4; ++j) {
    const int id0 = id_l + 256 * j;
    float4 x = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (vec) {
      // ld % 4 == 0 and id0 < V <= ld: the four floats lie inside the row
      if (id0 < V) x = *reinterpret_cast<const float4*>(row + id0);
    } else {
      if (id0 + 0 < V) x.x = row[id0 + 0];
      if (id0 + 1 < V) x.y = row[id0 + 1];
      if (id0 + 2 < V) x.z = row[id0 + 2];
      if (id0 + 3 < V) x.w = row[id0 + 3];
    }
    // what lies past V (padding columns, any bits) counts as -inf with an id above every token's
    v[j][0] = id0 + 0 < V ? x.x : -INFINITY;
    v[j][1] = id0 + 1 < V ? x.y : -INFINITY;
    v[j][2] = id0 + 2 < V ? x.z : -INFINITY;
    v[j][3] = id0 + 3 < V ? x.w : -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) mx = fmaxf(mx, v[j][e]);
  }
  mx = blk.max(mx);
  // z = x / temperature (a true division, monotone: max z = max x / temperature), -0 -> +0 so
  // that equal values have equal bits
  const float mz = mx / temperature + 0.0f;
  float s1 = 0.f, st = 0.f;
#pragma unroll
  for (int j = 0; j < NV4; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = v[j][e];
      s1 += x == -INFINITY ? 0.f : expf(x - mx);
      const float z = x / temperature + 0.0f;
      st += z == -INFINITY ? 0.f : expf(z - mz);
      // the registers hold the KEY of z through the top-k search (were they to hold z, the
      // compiler would carry the 64 loop-invariant keys beside them)
      v[j][e] = __uint_as_float(f2key(z));
    }
    ZS_ONE_AT_A_TIME();
  }
  s1 = blk.sum(s1);
  st = blk.sum(st);

  // the lowest id bound c such that exactly m of the values with bits tb have an id <= c
  auto tie_cut = [&](uint32_t tb, unsigned m) -> int {
    int c = 0;
#pragma unroll 1
    for (int bit = 1 << 16; bit > 0; bit >>= 1) {
      const int cand = c | bit, i0 = ids();
      uint32_t tb1 = tb;   // opaque per pass, or the 64 tie masks are kept in scalar registers
      asm volatile("" : "+v"(tb1));
      unsigned n = 0;
#pragma unroll
      for (int j = 0; j < NV4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          n += (__float_as_uint(v[j][e]) == tb1 && i0 + 256 * j + e < cand) ? 1u : 0u;
        ZS_ONE_AT_A_TIME();
      }
      if (blk.sum_u(n) < m) c = cand;
    }
    return c;   // the largest c with fewer than m ties below it: the m-th tie itself
  };

  // ---- top-k: t = the k-th largest key; kept = key > t, and the first (k - #greater) ties by id
  uint32_t tk_key = 0;
  int tk_cut = 0x7fffffff;
  const bool use_k = top_k > 0 && top_k < V;
  if (use_k) {
    uint32_t t = 0;
#pragma unroll 1
    for (uint32_t bit = 0x80000000u; bit > 0; bit >>= 1) {
      const uint32_t cand = t | bit;
      unsigned n = 0;
#pragma unroll
      for (int j = 0; j < NV4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) n += __float_as_uint(v[j][e]) >= cand ? 1u : 0u;
        ZS_ONE_AT_A_TIME();
      }
      if (blk.sum_u(n) >= (unsigned)top_k) t = cand;
    }
    unsigned ngt = 0, neq = 0;
#pragma unroll
    for (int j = 0; j < NV4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t k = __float_as_uint(v[j][e]);
        ngt += k > t ? 1u : 0u;
        neq += k == t ? 1u : 0u;
      }
      ZS_ONE_AT_A_TIME();
    }
    ngt = blk.sum_u(ngt);
    neq = blk.sum_u(neq);
    tk_key = t;
    const unsigned need = (unsigned)top_k - ngt;
    if (need < neq) tk_cut = tie_cut(t, need);
  }

  // ---- registers become p = exp(z - max z) for what is kept, -1 for what is not
  float sk = 0.f;
  const int i1 = ids();
#pragma unroll
  for (int j = 0; j < NV4; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int id = i1 + 256 * j + e;
      const uint32_t k = __float_as_uint(v[j][e]);
      const float z = key2f(k);
      bool keep = id < V;
      if (use_k) keep = keep && (k > tk_key || (k == tk_key && id <= tk_cut));
      const float p = z == -INFINITY ? 0.f : expf(z - mz);
      v[j][e] = keep ? p : -1.0f;
      sk += keep ? p : 0.f;
    }
    ZS_ONE_AT_A_TIME();
  }
  sk = blk.sum(sk);

  // ---- top-p over the bits of p (as a signed int: -1.0f sorts below every p >= 0)
  const float P = top_p * sk;
  if (top_p < 1.0f && P < sk) {
    int t = 0;
#pragma unroll 1
    for (int bit = 1 << 29; bit > 0; bit >>= 1) {   // p <= 1.0f = 0x3f800000 < 2^30
      const int cand = t | bit;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NV4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s += __float_as_int(v[j][e]) >= cand ? v[j][e] : 0.f;
        ZS_ONE_AT_A_TIME();
      }
      if (blk.sum(s) > P) t = cand;
    }
    float G = 0.f;
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j < NV4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = __float_as_int(v[j][e]);
        G += b > t ? v[j][e] : 0.f;
        n += b == t ? 1u : 0u;
      }
      ZS_ONE_AT_A_TIME();
    }
    G = blk.sum(G);
    n = blk.sum_u(n);
    const float tv = __int_as_float(t);
    // m = #{q < n : G + q tv <= P}; q = 0 always counts
    unsigned m = n;
    if (t > 0) {
      const float q = floorf((P - G) / tv);
      m = q < 0.f ? 1u : q >= (float)n ? n : (unsigned)q + 1u;
      while (m < n && G + (float)m * tv <= P) ++m;
      while (m > 1 && G + (float)(m - 1) * tv > P) --m;
    }
    int cut = 0x7fffffff;
    if (m < n) cut = tie_cut((uint32_t)t, m);
    const int i2 = ids();
#pragma unroll
    for (int j = 0; j < NV4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int b = __float_as_int(v[j][e]);
        const bool keep = b > t || (b == t && i2 + 256 * j + e <= cut);
        v[j][e] = keep ? v[j][e] : -1.0f;
      }
      ZS_ONE_AT_A_TIME();
    }
  }

  // ---- the draw: id-order prefix sum of the kept mass
  unsigned cnt = 0;
  float carry = 0.f;
#pragma unroll
  for (int j = 0; j < NV4; ++j) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s += v[j][e] >= 0.f ? v[j][e] : 0.f;
      cnt += v[j][e] >= 0.f ? 1u : 0u;
    }
    carry += __shfl(wave_incl_scan(s, lane), 63, 64);
  }
  cnt = blk.sum_u(cnt);          // (its barrier also orders wtot below after any earlier use)
  if (lane == 0) wtot[wid] = carry;
  __syncthreads();
  float wpre = 0.f, M = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    if (i == wid) wpre = M;
    M += wtot[i];
  }
  const int step = __hip_atomic_load(step_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t rid = row_id ? (uint32_t)row_id[r] : (uint32_t)r;
  const uint32_t w0 = philox_word0(rid, (uint32_t)step, 0u, 0u, seed_lo, seed_hi);
  const float target = (float)(((double)w0 + 0.5) * (1.0 / 4294967296.0) * (double)M);
  unsigned first = 0xffffffffu, last = 0u;
  carry = wpre;
  const int i3 = ids();
  float zero = 0.f;   // opaque: the second pass tests the values again (no 64 carried masks)
  asm volatile("" : "+v"(zero));
#pragma unroll
  for (int j = 0; j < NV4; ++j) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += v[j][e] >= zero ? v[j][e] : 0.f;
    const float incl = wave_incl_scan(s, lane);
    float run = carry + (incl - s);
    // (incl - s is not the exclusive sum bit for bit; any fixed rule serves: the token taken
    // is always a kept one, and a draw that such rounding could move is not decisive)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (v[j][e] >= zero) {
        const unsigned id = (unsigned)(i3 + 256 * j + e);
        run += v[j][e];
        if (run > target) first = ::min(first, id);
        last = id;
      }
    }
    carry += __shfl(incl, 63, 64);
  }
  unsigned tok = blk.min_u(first);
  if (tok == 0xffffffffu) tok = blk.max_u(last);   // uniform: every thread holds the same tok
  if (tid == 0) {
    const float x = row[tok];
    part_val[r] = x;
    part_idx[r] = (int)tok;
    if (logprob) logprob[r] = (x - mx) - logf(s1);
    if (kept) {
      kept[2 * (long)r + 0] = (float)cnt;
      kept[2 * (long)r + 1] = M / st;
    }
  }
}

template <int NV4>
static int launch(const float* logits, int R, int V, int ld, int vec, const int* row_id,
                  const int* step_ctr, long seed, float temperature, int top_k, float top_p,
                  float* part_val, int* part_idx, float* logprob, float* kept, hipStream_t st) {
  const uint64_t s = (uint64_t)seed;
  hipLaunchKernelGGL((sample_rows_kernel<NV4>), dim3((unsigned)R), dim3(NT), 0, st, logits, V, ld, vec,
                     row_id, step_ctr, (uint32_t)s, (uint32_t)(s >> 32), temperature, top_k, top_p,
                     part_val, part_idx, logprob, kept);
  ZS_LAUNCH_CHECK();
  return ZS_OK;
}

}  // namespace smp
}  // namespace zs

using namespace zs;

extern "C" int zs_sample_rows(const float* logits, int R, int V, int ld, const int* row_id,
                              const int* step_ctr, long seed, float temperature, int top_k,
                              float top_p, float* part_val, int* part_idx, float* logprob,
                              float* kept, void* stream) {
  ZS_REQUIRE(R > 0 && V >= 1 && V <= smp::MAX_V, "zs_sample_rows: R > 0 and 1 <= V <= %d", smp::MAX_V);
  ZS_REQUIRE(ld >= V, "zs_sample_rows: ld >= V");
  ZS_REQUIRE(temperature > 0.f && temperature <= 3.0e38f, "zs_sample_rows: temperature > 0 (finite)");
  ZS_REQUIRE(top_p > 0.f, "zs_sample_rows: top_p > 0");
  ZS_REQUIRE(top_k >= 0, "zs_sample_rows: top_k >= 0 (0 = off)");
  ZS_REQUIRE(logits && step_ctr && part_val && part_idx, "zs_sample_rows: null pointer");
  ZS_REQUIRE((((uintptr_t)logits | (uintptr_t)row_id | (uintptr_t)step_ctr | (uintptr_t)part_val |
               (uintptr_t)part_idx | (uintptr_t)logprob | (uintptr_t)kept) & 3) == 0,
             "zs_sample_rows: pointers must be 4-byte aligned");
  // rows of float4 when every row starts on 16 bytes, single floats otherwise
  const int vec = (((uintptr_t)logits & 15) == 0 && ld % 4 == 0) ? 1 : 0;
  hipStream_t st = S(stream);
  const int nv4 = cdiv(V, smp::NT * 4);
#define ZS_SAMPLE_CASE(N)                                                                        \
  if (nv4 <= N)                                                                                  \
    return smp::launch<N>(logits, R, V, ld, vec, row_id, step_ctr, seed, temperature, top_k, top_p, \
                          part_val, part_idx, logprob, kept, st)
  ZS_SAMPLE_CASE(1);
  ZS_SAMPLE_CASE(2);
  ZS_SAMPLE_CASE(4);
  ZS_SAMPLE_CASE(8);    // V <= 32768: Mistral's 32000
  ZS_SAMPLE_CASE(13);   // V <= 53248: GPT-2's 50257
  ZS_SAMPLE_CASE(16);
#undef ZS_SAMPLE_CASE
  return fail(ZS_ERR_ARG, "zs_sample_rows: V");
}
