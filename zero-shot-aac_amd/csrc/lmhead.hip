// The vocab-block family: GEMMs of M rows against a [N][K] matrix whose 128-column blocks are
// reduced in registers instead of being written out.
//   lmhead_kernel / lmhead_tile_kernel  per-block max / sum-exp / top-k (greedy argmax, beam
//                                       log-softmax top-k, get_prefix_tokens cosine argmax)
//   lmhead_nll_kernel                   the same statistics and top-1, plus a GIVEN token's logit
//   sim_rank_kernel                     the rank of given columns in each row (retrieval)
// All of them are thin shells over one core: vocab_tile (which block am I), transposed_product
// (the MFMA main loop) and the lane layout of its accumulators (acct_col / for_token_cols).
#include "gemm_fast.h"

namespace zs {

extern int g_fast_xcd;   // gemm.hip
extern int g_f32_fast;   // gemm.hip

constexpr int LM_BN = 128;
constexpr int MAXK = 8;
int g_lm_prio = 1;   // zs_tune_set("lm_prio", 0): LM head main loop without s_setprio

// ------------------------------------------------------------------ the shared core
struct VocabTile {
  int vb, mb, n0, m0, nblk;
};

// 1-D grid of nblk x ntm blocks.  XCD-local order: workgroup b runs on XCD b % 8; the remap
// gives each XCD a contiguous range of u, and u walks the row tiles fastest, so every row tile
// of a vocab block runs on the same XCD at about the same time: each 128-token W slice is
// fetched into one L2 once and reused by all row tiles (with the vocab block fastest, the
// 77 MB of W streamed once per row tile).
__device__ __forceinline__ VocabTile vocab_tile(int xcd_order, int M, int N, int BM) {
  const int ntm = cdiv(M, BM), nblk = cdiv(N, LM_BN), nwg = nblk * ntm;
  int vb, mb;
  if (xcd_order & 1) {
    const int b = blockIdx.x, x = b & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int u = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + (b >> 3);
    vb = u / ntm;
    mb = u - vb * ntm;
  } else {
    vb = blockIdx.x % nblk;
    mb = blockIdx.x / nblk;
  }
  return {vb, mb, vb * LM_BN, mb * BM, nblk};
}

// acct = W[n0 .. n0+128) x A[m0 .. m0+BM)^T on the LDS-DMA ring: the transposed product, W's rows
// (vocab, gallery) on the MFMA row axis, so a token's 128 values of this block sit in registers of
// one lane pair per wave row (LaneMap below).  f32 rows are staged as bf16 rows of twice the length
// (fast_compute F32); bf16 takes lean_mainloop when K % 64 == 0 (xcd_order & 2: s_setprio around
// the MFMA clusters, as gemm_lean_kernel).  `ssq` non-null: also each lane's half of the squared
// norm of its tokens, from the staged B fragments.  `smem` must be the kernel's ONE __shared__
// array (a second object can de-pipeline the DMA loop: DESIGN.md §5 item 4(a)).
template <typename T, int BM>
__device__ __forceinline__ void transposed_product(const T* A, int lda, int M, int m0, const T* W,
                                                   int ldw, int N, int n0, int K, int xcd_order,
                                                   char* smem,
                                                   f32x16_t (&acct)[LM_BN / 64][BM / 64],
                                                   float* ssq) {
  constexpr int E = sizeof(T) / 2;   // bf16 elements per element of T
  const bf16_t* a = (const bf16_t*)A;
  const bf16_t* w = (const bf16_t*)W;
  const DenseRows ra{a, E * lda, M, m0};
  const DenseRows rw{w, E * ldw, N, n0};
  if constexpr (sizeof(T) == 4) {
    if (ssq)
      fast_mainloop<LM_BN, BM, 2, 2, 2, 64, true, 0, true>(rw, ra, 0, 2 * K, smem, acct, 0, ssq);
    else
      fast_mainloop<LM_BN, BM, 2, 2, 2, 64, false, 0, true>(rw, ra, 0, 2 * K, smem, acct);
  } else if (K % 64 == 0) {
    if (ssq)
      lean_mainloop<LM_BN, BM, 2, 2, 2, 64, true>(w, ldw, N, n0, a, lda, M, m0, K, smem, acct, ssq);
    else if (xcd_order & 2)
      lean_mainloop<LM_BN, BM, 2, 2, 2, 64, false, true>(w, ldw, N, n0, a, lda, M, m0, K, smem,
                                                         acct);
    else
      lean_mainloop<LM_BN, BM, 2, 2, 2, 64>(w, ldw, N, n0, a, lda, M, m0, K, smem, acct);
  } else if (ssq) {
    fast_mainloop<LM_BN, BM, 2, 2, 2, 64, true>(rw, ra, 0, K, smem, acct, 0, ssq);
  } else {
    fast_mainloop<LM_BN, BM>(rw, ra, 0, K, smem, acct);
  }
}

// MFMA 32x32 accumulator layout: element e of 32-row tile i sits at this row of the wave's 64
__device__ __forceinline__ int acct_col(int i, int e, int lane) {
  return i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
}

// Where a lane's accumulators of the transposed product sit in the block: acct[i][j][e] is column
// n0 + wr0 + acct_col(i, e, lane) of token m0 + row(j).  The two lanes l and l ^ 32 hold the 64
// columns of one wave row of a token; the wave rows wg = 0, 1 hold the block's column halves.
template <int BM>
struct LaneMap {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr0 = (wid >> 1) * (LM_BN / 2), wc0 = (wid & 1) * (BM / 2), wg = wid >> 1;
  __device__ __forceinline__ int row(int j) const { return wc0 + j * 32 + (lane & 31); }
};

// f(column, value) over the 32 columns this lane holds of token row(j), in ascending column order
// (col0 = n0 + wr0).  i, j and e stay static indices: the accumulators never leave registers.
template <int BM, typename F>
__device__ __forceinline__ void for_token_cols(const f32x16_t (&acct)[LM_BN / 64][BM / 64], int j,
                                               int col0, int lane, F&& f) {
#pragma unroll
  for (int i = 0; i < LM_BN / 64; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) f(col0 + acct_col(i, e, lane), acct[i][j][e]);
}

// value descending, then index ascending (torch argmax / topk order)
__device__ __forceinline__ bool better(float v, int i, float w, int k) {
  return v > w || (v == w && i < k);
}

// Insert (v, n) into the descending list tv / ti; callers feed n in ascending order.  A value goes
// behind its equals (strict >), so the lower index stays first.  The list is descending, hence
// lt[q] = v > tv[q] is monotone in q and slot q takes v where lt[q] && !lt[q - 1], its upper
// neighbour where both hold: every entry behind the new one moves down one slot whatever it
// compares to.  (An earlier bubble compared the DISPLACED entry with strict > against its
// successor, so among equals the lower index slid behind the higher one or fell off the list.)
// Select-only (per-element branches became ~500 divergent exec-mask branches per kernel), all
// compares on the old list; the outer test skips a value no lane keeps.
template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&tv)[KMAX], int (&ti)[KMAX], float v, int n) {
  if (v > tv[KMAX - 1]) {
    bool lt[KMAX];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) lt[q] = v > tv[q];
#pragma unroll
    for (int q = KMAX - 1; q >= 1; --q) {
      tv[q] = lt[q] ? (lt[q - 1] ? tv[q - 1] : v) : tv[q];
      ti[q] = lt[q] ? (lt[q - 1] ? ti[q - 1] : n) : ti[q];
    }
    tv[0] = lt[0] ? v : tv[0];
    ti[0] = lt[0] ? n : ti[0];
  }
}

template <int KMAX>
__device__ __forceinline__ void topk_clear(float (&tv)[KMAX], int (&ti)[KMAX]) {
#pragma unroll
  for (int q = 0; q < KMAX; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
}

// merge with the partner lane's list (both lanes end with the same top-KMAX), select-only: the
// partner's entries bubble into this lane's list like new values (the same order as a merge)
template <int KMAX>
__device__ __forceinline__ void topk_merge_partner(float (&tv)[KMAX], int (&ti)[KMAX]) {
  float pv[KMAX];
  int pi[KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) { pv[q] = __shfl_xor(tv[q], 32, 64); pi[q] = __shfl_xor(ti[q], 32, 64); }
#pragma unroll
  for (int p = 0; p < KMAX; ++p) {
    float cv = pv[p];
    int ci = pi[p];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
      const bool c = better(cv, ci, tv[q], ti[q]);
      const float t = tv[q];
      const int u = ti[q];
      tv[q] = c ? cv : t;
      ti[q] = c ? ci : u;
      cv = c ? t : cv;
      ci = c ? u : ci;
    }
  }
}

// logits -> what the statistics see: * 1/||a|| (get_prefix_tokens), then / temp where temp != 1
// (generate2 / generate_beam's `temperature`, gpt2_prefix_eval.py:121, 196; a true division, as
// the reference)
struct LogitScale {
  float sc, temp;
  bool tdiv;
  // `real` false (a padding column): -inf, by a select
  __device__ __forceinline__ float operator()(float a, bool real = true) const {
    float v = real ? a * sc : -INFINITY;
    if (tdiv) v = v / temp;
    return v;
  }
};

// Softmax statistics of a 128-column block, one (max, sum-exp) pair per token.  put: a lane pair's
// sum of exp(logit - bv) over its 64 columns (bv: the pair's max; only when `want`) into the
// exchange area; merged: the block's pair from the two wave rows.
template <int BM>
struct BlockStats {
  float* xm;   // [2][BM] max
  float* xs;   // [2][BM] sum-exp
  static constexpr int BYTES = 2 * 2 * BM * 4;
  __device__ __forceinline__ explicit BlockStats(char* smem)
      : xm(reinterpret_cast<float*>(smem)), xs(xm + 2 * BM) {}
  __device__ __forceinline__ void put(const f32x16_t (&acct)[LM_BN / 64][BM / 64], int j, int col0,
                                      int V, const LaneMap<BM>& lm, const LogitScale& ls, float bv,
                                      bool want) const {
    float se = 0.f;
    if (want && bv != -INFINITY) {
      for_token_cols<BM>(acct, j, col0, lm.lane, [&](int n, float a) {
        if (n < V) se += __expf(ls(a) - bv);
      });
      se += __shfl_xor(se, 32, 64);
    }
    if (lm.lane < 32) {
      xm[lm.wg * BM + lm.row(j)] = bv;
      xs[lm.wg * BM + lm.row(j)] = se;
    }
  }
  __device__ __forceinline__ void merged(int r, float& g, float& se) const {
    const float m0v = xm[r], m1v = xm[BM + r];
    g = fmaxf(m0v, m1v);
    se = (m0v == -INFINITY ? 0.f : xs[r] * expf(m0v - g)) +
         (m1v == -INFINITY ? 0.f : xs[BM + r] * expf(m1v - g));
  }
};

// The register epilogue of the transposed product.  Per token: a descending top-KMAX list and the
// sum-exp over the lane's 32 vocab entries in registers, one xor-32 exchange with the partner
// lane, then the two waves holding the other 64 vocab rows of the same tokens merge through LDS
// (smem: the main loop's ring, free after the caller's barrier).  Ties keep the lower vocab index.
// part_stat == NULL (greedy argmax, get_prefix_tokens) skips the 64 exps per lane.
template <int BM, int KMAX>
__device__ __forceinline__ void topk_epilogue(const f32x16_t (&acct)[LM_BN / 64][BM / 64],
                                              const VocabTile& vt, int M, int V, bool row_norm,
                                              const float* ssq, float temp, int topk,
                                              float* part_stat, float* part_val, int* part_idx,
                                              char* smem) {
  const LaneMap<BM> lm{};
  const BlockStats<BM> st(smem);
  float* xv = reinterpret_cast<float*>(smem + st.BYTES);     // [2][BM][KMAX] top values
  int* xi = reinterpret_cast<int*>(xv + 2 * BM * KMAX);      // [2][BM][KMAX] top indices
  static_assert(BlockStats<BM>::BYTES + 2 * 2 * BM * KMAX * 4 <= 2 * FastTile<BM, LM_BN>::STAGE,
                "epilogue exchange fits the ring's LDS");
#pragma unroll
  for (int j = 0; j < BM / 64; ++j) {
    LogitScale ls{1.0f, temp, temp != 1.0f};
    if (row_norm) {
      const float t = ssq[j] + __shfl_xor(ssq[j], 32, 64);
      ls.sc = 1.0f / fmaxf(sqrtf(t), 1e-12f);
    }
    float tv[KMAX];
    int ti[KMAX];
    topk_clear(tv, ti);
    for_token_cols<BM>(acct, j, vt.n0 + lm.wr0, lm.lane, [&](int n, float a) {
      topk_insert(tv, ti, ls(a, n < V), n);
    });
    topk_merge_partner(tv, ti);
    st.put(acct, j, vt.n0 + lm.wr0, V, lm, ls, tv[0], part_stat != nullptr);
    if (lm.lane < 32) {
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        xv[(lm.wg * BM + lm.row(j)) * KMAX + q] = tv[q];
        xi[(lm.wg * BM + lm.row(j)) * KMAX + q] = ti[q];
      }
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r < BM; r += 256) {
    const int m = vt.m0 + r;
    if (m >= M) continue;
    const long o = (long)m * vt.nblk + vt.vb;
    if (part_stat != nullptr) {
      float g, se;
      st.merged(r, g, se);
      part_stat[o * 2 + 0] = g;
      part_stat[o * 2 + 1] = se;
    }
    const float* l0v = xv + r * KMAX;
    const int* l0i = xi + r * KMAX;
    const float* l1v = xv + (BM + r) * KMAX;
    const int* l1i = xi + (BM + r) * KMAX;
    int a = 0, b = 0;
    for (int q = 0; q < topk; ++q) {
      const bool ta = b >= KMAX || (a < KMAX && better(l0v[a], l0i[a], l1v[b], l1i[b]));
      part_val[o * topk + q] = ta ? l0v[a] : l1v[b];
      part_idx[o * topk + q] = ta ? l0i[a] : l1i[b];
      if (ta) ++a; else ++b;
    }
  }
}

// ------------------------------------------------------------------ LM head (+ row reductions)
// bf16 always, f32 with f32_fast 1: the ring main loop and the register epilogue
template <typename T, int BM, int KMAX>
__global__ __launch_bounds__(256) void lmhead_kernel(int xcd_order, int M, int K, int V, const T* A,
                                                     int lda, const T* W, int topk, int row_norm,
                                                     float* part_stat, float* part_val,
                                                     int* part_idx, float temp) {
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * FastTile<BM, LM_BN>::STAGE];
  const VocabTile vt = vocab_tile(xcd_order, M, V, BM);
  f32x16_t acct[LM_BN / 64][BM / 64];
  // per lane: its half of the squared norm of token wc0 + j*32 + (lane&31): the row norms for
  // get_prefix_tokens (normalize(a) . w == (a . w) / max(||a||, 1e-12))
  float ssq[BM / 64];
#pragma unroll
  for (int j = 0; j < BM / 64; ++j) ssq[j] = 0.f;
  if (row_norm)
    transposed_product<T, BM>(A, lda, M, vt.m0, W, K, V, vt.n0, K, xcd_order, smem_raw, acct, ssq);
  else
    transposed_product<T, BM>(A, lda, M, vt.m0, W, K, V, vt.n0, K, xcd_order, smem_raw, acct,
                              nullptr);
  __syncthreads();
  topk_epilogue<BM, KMAX>(acct, vt, M, V, row_norm, ssq, temp, topk, part_stat, part_val, part_idx,
                          smem_raw);
}

// f32 with f32_fast 0: the register-staged f32 main loop (product not transposed) and an
// epilogue that reduces the [BM][128] tile through LDS
template <typename T, int BM, int KMAX>
__global__ __launch_bounds__(256) void lmhead_tile_kernel(int xcd_order, int M, int K, int V,
                                                          const T* A, int lda, const T* W, int topk,
                                                          int row_norm, float* part_stat,
                                                          float* part_val, int* part_idx,
                                                          float temp) {
  const bool tdiv = temp != 1.0f;
  constexpr int LDW = BK + GemmTraits<T>::PAD;
  constexpr int TM = BM / 64, TN = LM_BN / 64;
  constexpr int SM = 2 * (BM + LM_BN) * LDW * (int)sizeof(T);
  static_assert(BM * (LM_BN + 1) * 4 <= SM && 2 * 256 * MAXK * 4 <= SM, "epilogue fits the loop's LDS");
  __shared__ __attribute__((aligned(16))) char smem_raw[SM + BM * 4];
  float* inv_norm = reinterpret_cast<float*>(smem_raw + SM);
  const VocabTile vt = vocab_tile(xcd_order, M, V, BM);
  const int n0 = vt.n0, m0 = vt.m0;
  f32x16_t acc[TM][TN];
  DenseA<T, BM> la{A, lda, M, m0};
  gemm_mainloop<T, BM, LM_BN>(la, W, K, V, n0, 0, K, (T*)smem_raw, acc);
  // row norms for get_prefix_tokens (normalize(a) . w == (a . w) / max(||a||, 1e-12))
  if (row_norm) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int r = wid; r < BM; r += 4) {
      float s = 0.f;
      if (m0 + r < M)
        for (int k = lane; k < K; k += 64) {
          float a = ldf(A + (long)(m0 + r) * lda + k);
          s += a * a;
        }
      s = wave_sum(s);
      if (lane == 0) inv_norm[r] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    }
  }
  __syncthreads();
  float* tile = reinterpret_cast<float*>(smem_raw);   // [BM][LM_BN+1]
  {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wr0 = (wid >> 1) * (BM / 2), wc0 = (wid & 1) * (LM_BN / 2);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e)   // rows on the MFMA row axis here: acct_col is a row
          tile[(wr0 + acct_col(i, e, lane)) * (LM_BN + 1) + wc0 + j * 32 + (lane & 31)] = acc[i][j][e];
  }
  __syncthreads();
  // each row is reduced by TPR threads, each scanning LM_BN/TPR consecutive columns
  constexpr int TPR = 256 / BM;
  constexpr int CPT = LM_BN / TPR;
  const int r = threadIdx.x / TPR, sub = threadIdx.x % TPR;
  const int m = m0 + r;
  const float scale = row_norm ? inv_norm[r] : 1.0f;
  float mx = -INFINITY;
  float tv[KMAX];
  int ti[KMAX];
  topk_clear(tv, ti);
  for (int c = sub * CPT; c < sub * CPT + CPT; ++c) {
    const int n = n0 + c;
    if (n >= V) break;
    float v = tile[r * (LM_BN + 1) + c] * scale;
    if (tdiv) v = v / temp;
    mx = fmaxf(mx, v);
    topk_insert(tv, ti, v, n);
  }
  // combine max across the TPR threads of this row (consecutive lanes)
  float gmx = mx;
#pragma unroll
  for (int o = 1; o < TPR; o <<= 1) gmx = fmaxf(gmx, __shfl_xor(gmx, o, 64));
  float se = 0.f;
  for (int c = sub * CPT; part_stat != nullptr && c < sub * CPT + CPT; ++c) {
    const int n = n0 + c;
    if (n >= V) break;
    se += expf((tdiv ? tile[r * (LM_BN + 1) + c] * scale / temp : tile[r * (LM_BN + 1) + c] * scale) - gmx);
  }
#pragma unroll
  for (int o = 1; o < TPR; o <<= 1) se += __shfl_xor(se, o, 64);
  __syncthreads();
  // merge the TPR sorted lists through LDS (reuse the tile area after the barrier)
  float* mv = reinterpret_cast<float*>(smem_raw);
  int* mi = reinterpret_cast<int*>(smem_raw + 256 * MAXK * 4);
#pragma unroll
  for (int q = 0; q < KMAX; ++q) { mv[threadIdx.x * MAXK + q] = tv[q]; mi[threadIdx.x * MAXK + q] = ti[q]; }
  __syncthreads();
  if (sub == 0 && m < M) {
    const long o = ((long)m * vt.nblk + vt.vb);
    if (part_stat != nullptr) {
      part_stat[o * 2 + 0] = gmx;
      part_stat[o * 2 + 1] = se;
    }
    int ptr[TPR];
#pragma unroll
    for (int t = 0; t < TPR; ++t) ptr[t] = 0;
    for (int q = 0; q < topk; ++q) {
      int best = -1;
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int t = 0; t < TPR; ++t) {
        if (ptr[t] >= topk) continue;
        const float v = mv[(threadIdx.x + t) * MAXK + ptr[t]];
        const int ix = mi[(threadIdx.x + t) * MAXK + ptr[t]];
        if (best < 0 || better(v, ix, bv, bi)) { best = t; bv = v; bi = ix; }
      }
      ptr[best]++;
      part_val[o * topk + q] = bv;
      part_idx[o * topk + q] = bi;
    }
  }
}

// ------------------------------------------------------------------ LM head, teacher-forced
// Scoring a GIVEN token per row (cross-entropy over the caption tokens: train_prompt.py:133,
// caption_model.py:297-313).  Per (row, 128-column block): the block's max, sum(exp(logit - max))
// and top-1 (value, index; ties -> lower index) -- lmhead_kernel's own epilogue at one list entry,
// so a row's log-sum-exp IS the one zs_lmhead_topk's partials give, bit for bit -- and, from the
// one lane of the one block that holds column tgt[m], the target's logit into tgt_logit[m]: one
// writer per row, no atomics.  No [M][V] logits.  Rows with tgt outside [0, V) write no target
// logit.
template <typename T, int BM>
__global__ __launch_bounds__(256) void lmhead_nll_kernel(int xcd_order, int M, int K, int V,
                                                         const T* A, int lda, const T* W,
                                                         const int* __restrict__ tgt,
                                                         float* __restrict__ part_stat,
                                                         float* __restrict__ part_val,
                                                         int* __restrict__ part_idx,
                                                         float* __restrict__ tgt_logit) {
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * FastTile<BM, LM_BN>::STAGE];
  const VocabTile vt = vocab_tile(xcd_order, M, V, BM);
  f32x16_t acct[LM_BN / 64][BM / 64];
  transposed_product<T, BM>(A, lda, M, vt.m0, W, K, V, vt.n0, K, xcd_order, smem_raw, acct, nullptr);
  __syncthreads();
  const LaneMap<BM> lm{};
#pragma unroll
  for (int j = 0; j < BM / 64; ++j) {
    const int m = vt.m0 + lm.row(j);
    const int t = m < M ? tgt[m] : -1;
    float tl = 0.f;
    bool hit = false;
    for_token_cols<BM>(acct, j, vt.n0 + lm.wr0, lm.lane, [&](int n, float a) {
      const bool h = n == t && n < V;
      tl = h ? a : tl;
      hit = hit || h;
    });
    if (hit) tgt_logit[m] = tl;        // t >= 0 here, so m < M
  }
  topk_epilogue<BM, 1>(acct, vt, M, V, false, nullptr, 1.0f, 1, part_stat, part_val, part_idx,
                       smem_raw);
}

// ------------------------------------------------------------------ similarity rank (retrieval)
// Retrieval metrics (a2t / t2a, retrieval/tools/utils.py:169-251) need, per query row m and target
// column j = tgt[m][t], the position of j in the row sorted by similarity: rank = #{n : sim[m][n] >
// sim[m][j]} + #{n < j : sim[m][n] == sim[m][j]} (value descending, then index ascending).
// The core with another register epilogue, launched twice so that every compared value -- the
// target's own included -- comes out of the same MFMA chain (an exact duplicate of the target row
// then compares EQUAL, whatever the rounding):
//   PASS 0  only the blocks whose 128 columns hold a target of one of their rows run the main
//           loop; the one lane that holds column tgt[m][t] writes tgt_sim[m][t] (one writer per
//           slot up to equal targets, which write the same bits).
//   PASS 1  every block counts, per (row, t), its columns that sort before the target; the lane
//           pair and the two wave rows are summed in registers / LDS and ONE integer atomicAdd per
//           (row, t, block) with a non-zero count goes to rank[m][t].  Integer sums commute: the
//           result does not depend on the order of the blocks.  No [M][N] matrix, no partials.
// Targets outside [0, N) count nothing (sim_rank_init_kernel has set their rank to -1).
__global__ void sim_rank_init_kernel(long total, int N, const int* __restrict__ tgt,
                                     float* __restrict__ tgt_sim, int* __restrict__ rank) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = tgt[i];
  const bool ok = j >= 0 && j < N;
  rank[i] = ok ? 0 : -1;
  if (!ok) tgt_sim[i] = 0.f;
}

template <typename T, int BM, int PASS>
__global__ __launch_bounds__(256) void sim_rank_kernel(int xcd_order, int M, int K, int N,
                                                       const T* Q, int ldq, const T* G, int ldg,
                                                       const int* __restrict__ tgt, int TT,
                                                       float* __restrict__ tgt_sim,
                                                       int* __restrict__ rank) {
  constexpr int SM_LOOP = 2 * FastTile<BM, LM_BN>::STAGE;   // 4 waves (2x2), 2 stages
  static_assert(BM * MAXK * 4 <= SM_LOOP, "epilogue exchange fits the ring's LDS");
  __shared__ __attribute__((aligned(16))) char smem_raw[SM_LOOP];
  const VocabTile vt = vocab_tile(xcd_order, M, N, BM);
  const int n0 = vt.n0, m0 = vt.m0;
  if constexpr (PASS == 0) {
    // a block none of whose rows has a target in its columns has nothing to store
    // (the vote goes through the ring's own LDS: ONE __shared__ array, see transposed_product)
    int* flag = reinterpret_cast<int*>(smem_raw);
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < BM * TT; i += 256) {
      const int m = m0 + i / TT;
      if (m < M) {
        const int j = tgt[(long)m0 * TT + i];
        if (j >= n0 && j < n0 + LM_BN && j < N) *flag = 1;
      }
    }
    __syncthreads();
    const int any = *flag;
    __syncthreads();                                   // read before the main loop's DMA lands
    if (!any) return;
  }
  f32x16_t acct[LM_BN / 64][BM / 64];
  transposed_product<T, BM>(Q, ldq, M, m0, G, ldg, N, n0, K, xcd_order, smem_raw, acct, nullptr);
  __syncthreads();
  constexpr int TNT = BM / 64;
  const LaneMap<BM> lm{};
  const int lane = lm.lane;
  int* xc = reinterpret_cast<int*>(smem_raw);               // [BM][MAXK] counts of wave row 1
  int cnt[TNT][MAXK];
#pragma unroll
  for (int j = 0; j < TNT; ++j) {
    const int m = m0 + lm.row(j);
    int tj[MAXK];
    float ts[MAXK];
#pragma unroll
    for (int t = 0; t < MAXK; ++t) {
      cnt[j][t] = 0;
      tj[t] = -1;
      ts[t] = INFINITY;
      if (t < TT && m < M) {
        const int c = tgt[(long)m * TT + t];
        if (c >= 0 && c < N) {
          tj[t] = c;
          if constexpr (PASS == 1) ts[t] = tgt_sim[(long)m * TT + t];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < MAXK; ++t) {
      if (t >= TT) break;                                  // uniform
      if constexpr (PASS == 0) {
        // the one accumulator element that holds column tj, if this lane has it (tj < N, so a
        // hit is a real column; tj = -1 hits nothing)
        float v = 0.f;
        bool mine = false;
        for_token_cols<BM>(acct, j, n0 + lm.wr0, lane, [&](int n, float cv) {
          const bool h = n == tj[t];
          v = h ? cv : v;
          mine = mine || h;
        });
        if (mine) tgt_sim[(long)m * TT + t] = v;           // tj >= 0 here, so m < M
      } else {
        int c = 0;
        for_token_cols<BM>(acct, j, n0 + lm.wr0, lane, [&](int n, float cv) {
          // before the target: a greater value, or an equal one at a lower index (n == tj
          // itself is neither); padding columns n >= N are not counted
          c += (n < N && (cv > ts[t] || (cv == ts[t] && n < tj[t]))) ? 1 : 0;
        });
        cnt[j][t] = c + __shfl_xor(c, 32, 64);
      }
    }
  }
  if constexpr (PASS == 1) {
    // the two wave rows hold column halves [0, 64) and [64, 128) of the block: add, then one
    // integer atomic per (query, t) of this block
    if (lm.wg == 1 && lane < 32) {
#pragma unroll
      for (int j = 0; j < TNT; ++j)
#pragma unroll
        for (int t = 0; t < MAXK; ++t) xc[lm.row(j) * MAXK + t] = cnt[j][t];
    }
    __syncthreads();
    if (lm.wg == 0 && lane < 32) {
#pragma unroll
      for (int j = 0; j < TNT; ++j) {
        const int r = lm.row(j);
        const int m = m0 + r;
#pragma unroll
        for (int t = 0; t < MAXK; ++t) {
          const int c = cnt[j][t] + xc[r * MAXK + t];
          if (t < TT && m < M && c != 0) atomicAdd(rank + (long)m * TT + t, c);
        }
      }
    }
  }
}

}  // namespace zs

using namespace zs;

// what every entry of the family asks of its two operands: A [M][lda], W [N][ldw], K columns used
static int lm_check(const char* fn, int M, int N, int K, int dtype, const void* A, int lda,
                    const void* W, int ldw) {
  ZS_REQUIRE(M > 0 && N > 0 && K > 0, "%s: bad shape", fn);
  ZS_REQUIRE(K % BK == 0 && lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K,
             "%s: K %% 32, leading dimensions %% 8 and >= K", fn);
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "%s: dtype", fn);
  ZS_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0,
             "%s: both matrices must be 16-byte aligned", fn);
  return 0;
}

// f(T, BM) with the family's row tile: 64 rows up to M = 64, 128 above
template <typename F>
static void lm_launch(int dtype, int M, F&& f) {
  using B64 = std::integral_constant<int, 64>;
  using B128 = std::integral_constant<int, 128>;
  if (M <= 64) {
    if (dtype == ZS_BF16) f(bf16_t{}, B64{}); else f(float{}, B64{});
  } else {
    if (dtype == ZS_BF16) f(bf16_t{}, B128{}); else f(float{}, B128{});
  }
}

static int lm_order() { return (g_fast_xcd ? 1 : 0) | (g_lm_prio ? 2 : 0); }

extern "C" int zs_lmhead_nblk(int V) { return cdiv(V, LM_BN); }

extern "C" int zs_lmhead_topk(int M, int K, int V, int dtype, const void* A, int lda,
                              const void* W, int topk, int row_norm, float* part_stat,
                              float* part_val, int* part_idx, void* stream) {
  return zs_lmhead_topk_t(M, K, V, dtype, A, lda, W, topk, row_norm, 1.0f, part_stat, part_val,
                          part_idx, stream);
}

extern "C" int zs_lmhead_topk_t(int M, int K, int V, int dtype, const void* A, int lda,
                                const void* W, int topk, int row_norm, float temperature,
                                float* part_stat, float* part_val, int* part_idx, void* stream) {
  ZS_REQUIRE(temperature > 0.f, "zs_lmhead_topk_t: temperature %g (> 0)", temperature);
  ZS_REQUIRE(!row_norm || temperature == 1.0f, "zs_lmhead_topk_t: row_norm with temperature");
  if (int rc = lm_check("zs_lmhead_topk", M, V, K, dtype, A, lda, W, K)) return rc;
  ZS_REQUIRE(topk >= 1 && topk <= MAXK, "zs_lmhead_topk: 1 <= topk <= 8");
  // f32 on the LDS-DMA ring unless f32_fast 0 (its 16-byte rows: lda % 8 and K % 32 hold)
  const bool ring = dtype == ZS_BF16 || g_f32_fast;
  lm_launch(dtype, M, [&](auto t, auto bm) {
    using T = decltype(t);
    constexpr int BM = decltype(bm)::value;
    // top-k lists of 1 (argmax), 5 (beam <= 5: generate_beam's default) or 8 entries per block
    auto go = [&](auto km) {
      constexpr int KM = decltype(km)::value;
      auto kernel = lmhead_kernel<T, BM, KM>;
      if constexpr (sizeof(T) == 4) {
        if (!ring) kernel = lmhead_tile_kernel<T, BM, KM>;
      }
      hipLaunchKernelGGL(kernel, dim3(cdiv(V, LM_BN) * cdiv(M, BM)), dim3(256), 0, S(stream),
                         lm_order(), M, K, V, (const T*)A, lda, (const T*)W, topk, row_norm,
                         part_stat, part_val, part_idx, temperature);
    };
    if (topk == 1) go(std::integral_constant<int, 1>{});
    else if (topk <= 5) go(std::integral_constant<int, 5>{});
    else go(std::integral_constant<int, 8>{});
  });
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_lmhead_nll(int M, int K, int V, int dtype, const void* A, int lda,
                             const void* W, const int* tgt, float* part_stat, float* part_val,
                             int* part_idx, float* tgt_logit, void* stream) {
  if (int rc = lm_check("zs_lmhead_nll", M, V, K, dtype, A, lda, W, K)) return rc;
  ZS_REQUIRE(A && W && tgt && part_stat && part_val && part_idx && tgt_logit,
             "zs_lmhead_nll: null pointer");
  lm_launch(dtype, M, [&](auto t, auto bm) {
    using T = decltype(t);
    constexpr int BM = decltype(bm)::value;
    hipLaunchKernelGGL((lmhead_nll_kernel<T, BM>), dim3(cdiv(V, LM_BN) * cdiv(M, BM)), dim3(256),
                       0, S(stream), lm_order(), M, K, V, (const T*)A, lda, (const T*)W, tgt,
                       part_stat, part_val, part_idx, tgt_logit);
  });
  ZS_LAUNCH_CHECK();
  return 0;
}

extern "C" int zs_sim_rank(int M, int N, int K, int dtype, const void* Q, int ldq, const void* G,
                           int ldg, const int* tgt, int T, float* tgt_sim, int* rank,
                           void* stream) {
  if (int rc = lm_check("zs_sim_rank", M, N, K, dtype, Q, ldq, G, ldg)) return rc;
  ZS_REQUIRE(T >= 1 && T <= MAXK, "zs_sim_rank: 1 <= T <= 8");
  ZS_REQUIRE(Q && G && tgt && tgt_sim && rank, "zs_sim_rank: null pointer");
  const long total = (long)M * T;
  const int nblk = cdiv(N, LM_BN);
  // M x T and the 1-D grid of the 64-row tile must fit an int
  ZS_REQUIRE(total < (1L << 31) && (long)nblk * cdiv(M, 64) < (1L << 31),
             "zs_sim_rank: M x T or the grid does not fit an int");
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(sim_rank_init_kernel, dim3((unsigned)cdiv(total, 256L)), dim3(256), 0, st,
                     total, N, tgt, tgt_sim, rank);
  ZS_LAUNCH_CHECK();
  hipError_t err = hipSuccess;
  lm_launch(dtype, M, [&](auto t, auto bm) {
    using E = decltype(t);
    constexpr int BM = decltype(bm)::value;
    auto pass = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(nblk * cdiv(M, BM)), dim3(256), 0, st, lm_order(), M, K, N,
                         (const E*)Q, ldq, (const E*)G, ldg, tgt, T, tgt_sim, rank);
      return hipGetLastError();
    };
    err = pass(sim_rank_kernel<E, BM, 0>);
    if (err == hipSuccess) err = pass(sim_rank_kernel<E, BM, 1>);
  });
  ZS_CHECK_HIP(err);
  return 0;
}
