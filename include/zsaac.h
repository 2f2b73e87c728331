/*
 * zsaac.h — C-ABI of libzsaac_hip.so, the MI355X (gfx950) kernels behind the zero-shot audio
 * captioning hot path of XinMing0411/zero-shot-AAC.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator); the
 *     library never allocates or frees caller memory;
 *   - shapes/strides are explicit ints, element strides (not bytes);
 *   - `dtype` selects the storage/compute type of weights and GEMM operands:
 *       ZS_F32  = parity mode (f32 operands, exact-f32 MFMA 32x32x2f32, f32 accumulate)
 *       ZS_BF16 = perf mode   (bf16 operands, MFMA 32x32x16 bf16, f32 accumulate)
 *     residual streams, softmax, LayerNorm statistics and all reductions are f32 in both modes;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); every launch is
 *     stream-ordered, allocation-free and sync-free, so a caller may capture it into a hipGraph;
 *   - return 0 on success or a negative zs_status; zs_last_error() gives a thread-local message.
 *
 * Each entry point names the reference code it replaces (paths under the reference repo root).
 */
#ifndef ZSAAC_H
#define ZSAAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum zs_status { ZS_OK = 0, ZS_ERR_ARG = -1, ZS_ERR_DTYPE = -2, ZS_ERR_HIP = -3, ZS_ERR_UNSUPPORTED = -4 };
enum zs_dtype { ZS_F32 = 0, ZS_BF16 = 1 };
enum zs_act { ZS_ACT_NONE = 0, ZS_ACT_GELU_ERF = 1, ZS_ACT_GELU_TANH = 2, ZS_ACT_RELU = 3, ZS_ACT_TANH = 4 };

/* ------------------------------------------------------------------ runtime */
int zs_version(void);                         /* ABI version, bumped on signature change */
int zs_last_error(char* buf, size_t len);     /* copies the thread-local last error message */
int zs_device_arch(char* buf, size_t len);    /* gcnArchName of the current device (e.g. gfx950) */
int zs_tune_set(const char* key, int value);  /* tuning knobs, e.g. "skinny_mode" (0 fence, 1 sc1) */
/* zs_stream_create: a new non-blocking HIP stream, bound to its hardware queue at once (ROCclr
 * assigns queues round-robin at a stream's first dispatch), so streams created back to back run
 * on distinct hardware queues while GPU_MAX_HW_QUEUES allows.  Used for the concurrent batch
 * streams (two streams sharing a hardware queue serialize).  priority < 0: the device's highest
 * stream priority, > 0: its lowest, 0: the default. */
int zs_stream_create(void** stream, int priority);
/* zs_stream_create_masked: the same, restricted to the CUs whose bits are set in cu_mask
 * (mask_words 32-bit words, bit i = CU i, hipExtStreamCreateWithCUMask): the caption runner's
 * optional split of the chip between the begins (prompt .. step 0) and the decode grids. */
int zs_stream_create_masked(void** stream, const unsigned* cu_mask, int mask_words);
int zs_stream_destroy(void* stream);
/* zs_stream_spin: enqueue a one-wave kernel that holds `stream` for `us` microseconds (s_memrealtime,
 * 100 MHz; nothing written): the caption runner releases the first wave of persistent decode grids
 * one after another, 200 us apart, after a gate they all wait on -- released together, the
 * dispatcher sometimes left one grid without room for all its workgroups until another grid
 * ended (a grid ~40 ms late; profiles/r6/begin_first_ab.txt).  0 <= us <= 1e6; us == 0 enqueues
 * nothing. */
int zs_stream_spin(int us, void* stream);

/* ------------------------------------------------------------------ audio front end
 * zs_logmel: retrieval/models/feature_extractor.py:34-38 (torchlibrosa Spectrogram +
 * LogmelFilterBank, n_fft 1024, hop 320, hann, center/reflect, power 2, 64 Slaney mels,
 * 10*log10(max(x,1e-10))) fused with bn0 (htsat.py:949-951 / cnns.py:176-178):
 *   wav [B][T] f32 -> out [B][n_frames][64] f32, n_frames = T/hop + 1.
 * window[1024], twiddle[1024] = (cos, sin)(-2*pi*k/1024) interleaved for k < 512 (the DFT is a
 * radix-4 FFT in LDS, two real frames packed per complex FFT), melW[64][513] (librosa.filters.mel, row m nonzero on
 * [mel_lo[m], mel_hi[m])), bn_{mean,var,weight,bias}[64] (eval BatchNorm, eps 1e-5; pass NULL
 * bn_mean to skip bn0).  Accepts B > 0, T > 512 (the reflection reads sample 512), B * n_frames
 * within an int; every other buffer non-NULL. */
int zs_logmel(const float* wav, int B, int T, const float* window, const float* twiddle,
              const float* melW,
              const int* mel_lo, const int* mel_hi, const float* bn_mean, const float* bn_var,
              const float* bn_weight, const float* bn_bias, float* out, void* stream);

/* zs_wav2img: htsat.py:908-923 reshape_wav2img — bicubic (A=-0.75, align_corners=True) resize of
 * the time axis T_in -> 1024 and fold (B,1,1024,64) -> (B,256,256).  in [B][T_in][64] f32.
 * Accepts 0 < B <= 32767 (B * 65536 within an int), 1 < T_in <= 1024 (T_in = 1024 copies);
 * non-NULL buffers. */
int zs_wav2img(const float* in, int B, int T_in, float* img, void* stream);

/* zs_pack_clips: ragged mono clips (clip b = flat[offsets[b] .. offsets[b] + lengths[b])) ->
 * out [B][T] f32: each cropped to its first T samples or zero-padded at the end, exactly as
 * data_handing/embeddings_generator.py:53-59 fits clips to max_length * sr before encode_audio.
 * T % 4 == 0; out 16-byte aligned. */
int zs_pack_clips(const float* flat, const long* offsets, const int* lengths, int B, int T,
                  float* out, void* stream);

/* zs_resample_pack: data_handing/embeddings_generator.py:48-59 from decoded files --
 * librosa.load(path, sr=sr_out, mono=True) and the crop / pad to T -- in one launch per 64 clips:
 * clip b is n_frames[b] interleaved frames of channels[b] channels at sr_in[b] Hz, starting at
 * element offsets[b] of the flat device buffer `frames` (fmt 0: f32, 1: s16, read as x / 32768).
 * out [B][T] f32: row b is librosa.to_mono (np.mean over the channels, f32) resampled with
 * resampy's resample_f to sr_out (librosa 0.9.2's res_type "kaiser_best"), its first
 * min(n_out[b], T) outputs; every later element of the row is 0.  n_out[b] is resampy's output
 * length int(n_frames * (sr_out / sr_in)) of the WHOLE file, so n_frames[b] may be a prefix of it
 * (the first T outputs read ceil(T sr_in / sr_out) + wing + 1 frames).  sr_in[b] == sr_out is
 * the downmix alone, bit-exact (librosa does not resample then).
 * table [num_zeros << precision | 1][2] f32 on the device, 8-byte aligned: (win[i], win[i+1] -
 * win[i]) of resampy's half filter, the last delta 0; kaiser_best is num_zeros 64, precision 9.
 * Output t sits at input time t sr_in / sr_out, held as the 64-bit integer quotient and
 * remainder of t * sr_in by sr_out (exact at any t).
 * offsets, n_frames, channels, sr_in and n_out are HOST arrays [B] (they are validated here and
 * travel as kernel arguments: no copy, no synchronisation).  Accepts B > 0, T > 0, fmt 0 | 1,
 * 1 <= channels <= 8, 1 <= sr <= 2^24, sr_in <= 8 sr_out, sr_out <= 8 sr_in, a table step
 * int(min(1, sr_out / sr_in) << precision) >= 1, non-NULL pointers; anything else is refused
 * before the first launch. */
int zs_resample_pack(const void* frames, int fmt, const long* offsets, const int* n_frames,
                     const int* channels, const int* sr_in, const int* n_out, int B, int sr_out,
                     int T, const float* table, int num_zeros, int precision, float* out,
                     void* stream);

/* zs_resample_windows: zs_resample_pack for recordings longer than T -- each recording is
 * resampled once, straight into overlapping window rows.  The R recordings lie in `frames` as
 * zs_resample_pack's clips do (offsets, n_frames, channels, sr_in, n_out: HOST arrays [R],
 * validated here, kernel arguments; n_frames[r] is the WHOLE recording).  n_win[r] (host) is the
 * number of window rows of recording r (zsaac.longform.window_plan; 0 writes no row).
 * out [sum n_win][T] f32, recording-major: with row0[r] = sum of n_win before r,
 *   out[row0[r] + w][t] = y_r[w * hop + t]   for w * hop + t < n_out[r], else exactly +0,
 * y_r the signal zs_resample_pack writes for recording r with an unbounded T (downmix,
 * kaiser_best, gain; the downmix alone at sr_in == sr_out).  The arithmetic of an output depends
 * on its global index w * hop + t alone (held in 64 bits), so a window row is bit-equal to the
 * same outputs of a zs_resample_pack row, whatever hop.
 * One launch per 64 recordings (and per 65535 window rows); a block finds its recording from
 * the per-recording row0 of its descriptor.
 * Refuses, before the first launch and with `out` untouched, everything zs_resample_pack
 * refuses and: hop <= 0; n_win[r] < 0; a last window without a valid output ((n_win[r] - 1) *
 * hop >= max(n_out[r], 1) for n_win[r] > 1); a last input index n_out * sr_in / sr_out that does
 * not fit an int; sum n_win not an int or sum n_win * T not a long. */
int zs_resample_windows(const void* frames, int fmt, const long* offsets, const int* n_frames,
                        const int* channels, const int* sr_in, const int* n_out, const int* n_win,
                        int R, int sr_out, int T, int hop, const float* table, int num_zeros,
                        int precision, float* out, void* stream);

/* zs_window_stitch: the windows' head outputs back onto one time line per recording (the back
 * of the windowed pass zs_resample_windows starts).  Device tables: plan [R][4] int32 = (row0,
 * n_win, frow0, F) per recording -- its first window row, its windows, its first time-line row
 * and its time-line frames, frow0 ascending with frow0[r + 1] = frow0[r] + F[r] -- and wgt [W]
 * f32, window row i's share of valid samples v / T.  Window w's head frame j is time-line frame
 * w * hop_f + j (hop_f = hop / (T / 32) head frames).
 *   timeline[frow0 + f][k] (k < N) = the mean over the windows w with 0 <= f - w * hop_f < 32 of
 *     frame[row0 + w][f - w * hop_f][k]: added in ascending w in f32, then divided by their
 *     count c (1 <= c <= ceil(32 / hop_f)); c == 1 copies the value.
 *   rec_clip[r][k] = max_w clip[row0 + w][k] for k < N; columns [N, ldrc) are written -inf, so
 *     with ldrc % 8 == 0 zs_sim_topk_finalize(rec_clip, idx, R, ldrc / 8, 8, k, ...) is the
 *     recording's top-k.
 *   rec_emb[r][0..K) = s / max(||s||, 1e-12), s = sum_w wgt[row0 + w] * emb[row0 + w] in
 *     ascending w in f32 (product rounded, then added), the norm reduced in zs_l2norm_rows'
 *     order; n_win == 1 copies the row bit for bit.
 * frame [W][32][ldf], clip [W][ldc], emb [W][lde], timeline [sum F][ldt], rec_clip [R][ldrc],
 * rec_emb [R][ldre], all f32; an input / output pair may be NULL.  Only columns [0, N) of a
 * time-line row and [0, K) of an embedding row are written.  16-byte accesses where ldf and ldt
 * are multiples of 4 and frame / timeline 16-byte aligned, scalar ones otherwise.  No atomics,
 * fixed orders: a recording's outputs are bit-identical whatever R and whichever recordings
 * share the launch.
 * Refuses before any launch: R <= 0; hop_f outside [1, 32]; N <= 0; a leading dimension below
 * N (frame, clip, timeline, rec_clip) or K (emb, rec_emb); K not a multiple of 32 or > 2048; a
 * NULL plan / wgt (plan 16-byte aligned); an output without its input; no output at all.  The
 * plan's contents are the host's to check when it builds it (zsaac.longform.stitch_tables). */
int zs_window_stitch(const int* plan, const float* wgt, int R, int hop_f, int N,
                     const float* frame, int ldf, const float* clip, int ldc, const float* emb,
                     int lde, int K, float* timeline, int ldt, float* rec_clip, int ldrc,
                     float* rec_emb, int ldre, void* stream);

/* zs_patch_embed: htsat.py:115-125 PatchEmbed (Conv2d 1->96, k4 s4) + LayerNorm(96):
 * img [B][256][256] f32 -> x [B*4096][96] f32 (token = row*64 + col of the 64x64 patch grid).
 * Accepts 0 < B <= 32767; non-NULL buffers. */
int zs_patch_embed(const float* img, int B, const float* w /*[96][16]*/, const float* b,
                   const float* ln_w, const float* ln_b, float* x, void* stream);

/* ------------------------------------------------------------------ generic building blocks
 * zs_layernorm: y[m] = LN(x[rows ? rows[m] : m]) * w + b over C (eps), x f32, y in `ydtype`
 * (ZS_F32/ZS_BF16).  `rows` (int32, may be NULL) gathers rows, e.g. GPT-2 ln_f on the last
 * prompt position of every ragged row (an index may repeat).  M >= 0 (M == 0 does nothing),
 * C > 0, ldx >= C, ldy >= C.  Any C, leading dimension and alignment is accepted: rows of
 * C % 4 == 0, C <= 1024 with ldx % 4 == ldy % 4 == 0 and x, w, b 16-byte (y: 16-byte f32, 8-byte
 * bf16) aligned take the one-pass register kernel, everything else the strided kernel. */
int zs_layernorm(const float* x, int M, int C, int ldx, const int* rows, const float* w,
                 const float* b, float eps, void* y, int ldy, int ydtype, void* stream);

/* zs_gemm: out[m][n] = act(sum_k A[m][k] * W[n][k] + bias[n]) + residual[m][n]
 *   A [M][lda], W [N][ldw] in `dtype`; bias f32 or NULL; residual f32 [M][ldr] or NULL (may alias
 *   out); out in `out_dtype`.  K % 32 == 0.  split_k > 1 needs a f32 workspace of
 *   split_k*M*N floats (deterministic slab reduction, no atomics; its contents on entry do not
 *   matter).  split_k == 0 = auto: bf16 M <= 64 takes the row-group kernel (no workspace) at the
 *   K it covers (256, 512, 768, 1024, 1536, 2048, 3072, 3840, 4096); otherwise, for M <= 64 (and
 *   up to 256 rows for f32, or bf16 with K >= 2048 on a small grid) and K % 64 == 0, a
 *   weight-streaming split-K kernel whose last-arriving workgroup reduces the slabs in order
 *   (deterministic); it needs a workspace of zs_gemm_workspace_floats(M,N,K) floats
 *   ZEROED ONCE at allocation (its tile counters re-arm themselves); without one, the tiled kernel.
 *   Accepts: M >= 0 (M == 0: nothing is done), any N > 0; lda >= K and ldw >= K, both multiples of
 *   8 ELEMENTS, A and W 16-byte aligned; only columns [0, K) of rows [0, M) / [0, N) are read, so
 *   padding columns and rows behind them may hold anything, NaN included.  ldo >= N, ldr >= N and
 *   the alignment of out, residual and bias are free: 16-byte aligned bases with ldo % 8 == 0
 *   (ldr % 4 == 0) take vector stores (loads), everything else the scalar paths, with the same
 *   result; only columns [0, N) of rows [0, M) of out are written.
 *   Refuses (ZS_ERR_ARG, nothing launched): M < 0, N <= 0, K <= 0, K % 32 != 0, lda or ldw not a
 *   multiple of 8 or smaller than K, A or W not 16-byte aligned, split_k < 0, split_k > 1 without
 *   a workspace, a dtype other than ZS_F32 / ZS_BF16.
 *   Replaces every nn.Linear / HF Conv1D on the path (Conv1D weights are repacked to [N][K]). */
int zs_gemm(int M, int N, int K, int dtype, const void* A, int lda, const void* W, int ldw,
            const float* bias, const float* residual, int ldr, void* out, int ldo, int out_dtype,
            int act, int split_k, float* workspace, void* stream);

int zs_gemm_workspace_floats(int M, int N, int K);

/* zs_gemm_ln: out[m][n] = act(sum_k LN(x[m])[k] * W[n][k] + bias[n]) + residual[m][n] for
 *   M <= 64 rows (the GPT-2 decode step at the reference's eval batch of 64): LayerNorm over K
 *   (eps; ln_w / ln_b f32) of the f32 rows x [M][ldx], rounded to bf16, times bf16 W [N][ldw].
 *   ln_w == ln_b == NULL: normalise only (the caller folded the affine into W and bias).
 *   Replaces the ln_1 -> attn.c_attn and ln_2 -> mlp.c_fc launch pairs of transformers'
 *   GPT2Block (the zs_layernorm + zs_gemm sequence).  One launch, no workspace.
 *   Accepts: 1 <= M <= 64, K 768 or 1024, any N > 0; ldx % 4 == 0, ldw % 8 == 0, ldx >= K,
 *   ldw >= K; x, ln_w, ln_b and W 16-byte aligned; only columns [0, K) of x and W are read.  ldo, ldr and the alignment
 *   of out, residual and bias are free (as zs_gemm).  Everything else is refused before a launch. */
int zs_gemm_ln(int M, int N, int K, const float* x, int ldx, const float* ln_w, const float* ln_b,
               float eps, const void* W, int ldw, const float* bias, const float* residual,
               int ldr, void* out, int ldo, int out_dtype, int act, void* stream);

/* zs_gemm_ln_f32: zs_gemm_ln with f32 W [N][ldw] and f32 out (the f32 parity mode's decode
 *   step): LayerNorm of the f32 rows x with the affine (ln_w, ln_b) applied in f32 (no rounding
 *   of the normalised rows), exact f32 products and f32 accumulation (v_mfma_f32_16x16x4_f32).
 *   1 <= M <= 64, K 768 or 1024; ldx % 4 == 0, ldw % 4 == 0, ldx >= K, ldw >= K; x, W and the
 *   LN params 16-byte aligned (anything else is refused before a launch); ldo, ldr and the
 *   alignment of out, residual and bias are free.  Replaces GPT2Block's
 *   ln_1 -> c_attn / ln_2 -> c_fc pairs.
 *   ln_w == ln_b == NULL: no LayerNorm at all (out = act(x W^T + b) + residual, K 768, 1024 or
 *   3072: the attn.c_proj / mlp.c_proj of the same step); there is no normalise-only mode here.
 *   zs_gemm keeps its own f32 kernels, so a row's zs_gemm result stays independent of how many
 *   rows share the launch. */
int zs_gemm_ln_f32(int M, int N, int K, const float* x, int ldx, const float* ln_w,
                   const float* ln_b, float eps, const float* W, int ldw, const float* bias,
                   const float* residual, int ldr, float* out, int ldo, int act, void* stream);

/* zs_l2norm_rows: y = x / max(||x||_2, eps) per row (F.normalize, ase_model.py:54). in-place ok */
int zs_l2norm_rows(const float* x, int M, int C, float eps, float* y, void* stream);

/* ------------------------------------------------------------------ HTSAT
 * zs_window_attention: htsat.py:312-347 W-MSA/SW-MSA for one SwinTransformerBlock, with the
 * cyclic roll (htsat.py:443-463), window partition/reverse and the -100 shift mask (406-425)
 * folded into the indexing.  qkv [B*H*W][3C] (dtype) in natural token order; out [B*H*W][C]
 * (dtype) in natural token order.  head_dim = C/heads (24 in HTSAT), ws*ws == 64.
 * rel_table [(2ws-1)^2][heads] f32.
 * Accepts ws == 8, H and W multiples of 8 (H != W allowed), 0 <= shift < 8, C % heads == 0,
 * B*H*W within an int, non-NULL buffers.  Head dims: ZS_BF16 8, 16, 24, 32 (MFMA kernel; with
 * zs_tune_set("window_mfma", 0) only 24 and 32), ZS_F32 24 and 32; any other head dim returns
 * ZS_ERR_UNSUPPORTED. */
int zs_window_attention(const void* qkv, int B, int H, int W, int C, int heads, int ws, int shift,
                        const float* rel_table, void* out, int dtype, void* stream);

/* zs_swin_block: one whole SwinTransformerBlock (htsat.py:427-474, eval) in ONE launch, bf16
 * operands / f32 residual: x += proj(WindowAttention(LN1(x))); x += fc2(GELU(fc1(LN2(x)))),
 * with the roll, window partition/reverse, rel-pos bias and -100 shift mask folded in (replaces
 * the zs_layernorm / zs_gemm / zs_window_attention sequence of one block).  One workgroup per
 * 8x8 window.  x [B*H*W][C] f32, updated in place.  C in {96, 192, 384}, heads = C / 24.
 * Weights are fragment-packed bf16 (see csrc/swin.hip): frag(nt, ks)[lane][j] =
 * W[16 nt + lane%16][32 ks + 8 (lane/16) + j], stored [N/16][K/32][64][8]:
 *   wqkv_packed: qkv.weight regrouped per group of G heads (G = 2 for C <= 192, 4 for C = 384)
 *   as rows [q h0..h(G-1), k h0.., v h0..] x 32 (head dim 24 zero-padded to 32) =
 *   [heads/G][96 G][C], then packed;  bqkv_packed [heads/G][96 G] f32 (same order, zero pad);  wproj [C][C], w1 [4C][C],
 *   w2 [C][4C] packed;  biases / LayerNorm params f32;  rel_table [225][heads] f32. */
int zs_swin_block(float* x, int B, int H, int W, int C, int heads, int shift, const float* ln1_w,
                  const float* ln1_b, const void* wqkv_packed, const float* bqkv_packed,
                  const float* rel_table, const void* wproj_packed, const float* bproj,
                  const float* ln2_w, const float* ln2_b, const void* w1_packed, const float* b1,
                  const void* w2_packed, const float* b2, void* stream);

/* zs_patch_merge_ln: htsat.py:492-511 gather x0..x3 of each 2x2 patch + LayerNorm(4C):
 * x [B][H][W][C] f32 -> y [B*(H/2)*(W/2)][4C] (dtype); the reduction Linear is a zs_gemm.
 * Accepts B > 0, even H and W (H != W allowed), any C > 0, B*H*W within an int. */
int zs_patch_merge_ln(const float* x, int B, int H, int W, int C, const float* ln_w,
                      const float* ln_b, void* y, int dtype, void* stream);

/* zs_ln_meanpool: htsat.py:830,838-847 final LayerNorm + mean over the N tokens -> [B][C] f32.
 * x [B][N][C] f32.  B, N > 0; 0 < C <= min(2048, L / 64) where L is the device's LDS limit per
 * workgroup in bytes (hipDeviceAttributeMaxSharedMemoryPerBlock: the kernel keeps 16 x C f32
 * partial sums in dynamic LDS).  gfx950 reports 160 KiB, so C <= 2048 there; a 64 KiB device
 * accepts C <= 1024.  A larger C is refused with ZS_ERR_ARG, never launched. */
int zs_ln_meanpool(const float* x, int B, int N, int C, const float* ln_w, const float* ln_b,
                   float* out, void* stream);

/* ------------------------------------------------------------------ HTSAT tagging head
 * htsat.py:830-894 (forward_features past the last stage): clip-level tags and frame-level sound
 * events from the tokens zs_ln_meanpool reads.  Token n = f * 8 + t (frequency row f, time
 * column t, an 8 x 8 map); the reference regroups it (834-839) into 32 time frames tau of 2
 * frequency bins c:  tok(tau, c) = (2 (tau / 8) + c) * 8 + tau % 8.
 *
 * zs_tag_prep: htsat.py:830 (`norm`, eps 1e-5) and 834-847 up to `fine_grained_latent_output`
 * before its x32 repeat, in one pass over x [B][64][C] f32:
 *   xn [B][64][C] (dtype) = LayerNorm(x), the operand of zs_tag_conv;
 *   fine [B][32][C] f32, fine[b][tau] = (xn[b][tok(tau, 0)] + xn[b][tok(tau, 1)]) / 2 taken from
 *   the f32 xn before any rounding to bf16.
 * Accepts B > 0 (B * 64 rows), C a multiple of 32 with C <= 2048, dtype ZS_F32 or ZS_BF16,
 * non-NULL buffers; everything else is refused before any launch with the outputs untouched. */
int zs_tag_prep(const float* x, int B, int C, const float* ln_w, const float* ln_b, void* xn,
                int dtype, float* fine, void* stream);

/* zs_tag_conv: htsat.py:849-894, `tscam_conv` = Conv2d(C, N, (2, 3), padding (0, 1)) over the
 * (bin, frame) map, flatten, sigmoid, and the clip-level sigmoid of the time mean -- replacing the
 * reference's reshape / permute / conv2d / interpolate sequence without an im2col matrix:
 *   z[b][tau][k]   = bias[k] + sum_{c<2} sum_{d<3} sum_ch W[k][ch][c][d] xn[b][tok(tau+d-1, c)][ch]
 *                    (terms with tau + d - 1 outside [0, 32) are zero)
 *   frame[b][tau][k] = sigmoid(z)              [B][32][ldf] f32 (`framewise_output` before x32)
 *   clip[b][k]       = sigmoid(mean_tau z)     [B][ldc] f32     (`clipwise_output`)
 *   logits (may be NULL) = z, in frame's layout.
 * Only columns [0, N) of a row are written.  xn [B][64][C] (dtype, from zs_tag_prep).  w_packed
 * (dtype): the weight as a [Np][6 C] matrix, Np = N rounded up to 16 with zero rows past N,
 * column (c * 3 + d) * C + ch = W[k][ch][c][d], in swin.hip's fragment packing
 * [Np/16][6C/32][64][8]: frag(nt, ks)[lane][j] = W[16 nt + lane % 16][32 ks + 8 (lane / 16) + j].
 * ZS_BF16: bf16 MFMA with f32 accumulation; ZS_F32: f32 MFMA (exact f32 products, summed 64
 * at a time into a fresh accumulator that is then added to the total).  One
 * workgroup per (clip, 128 classes): the time mean is tile-local, no atomics, every reduction in
 * a fixed order -- a clip's outputs are bit-identical whatever B and whichever clips share the
 * launch, and two equal weight rows give bit-equal columns.  With ldc a multiple of 8 and the
 * padding of clip holding -inf, zs_sim_topk_finalize(clip, idx, B, ldc / 8, 8, k, ...) is the
 * row's top-k (idx [B][ldc]: 0 .. N-1, then 0x7fffffff).
 * Accepts 0 < B <= 65535, C a multiple of 32 with C <= 2048, 0 < N <= 2^20, ldf >= N,
 * ldc >= N, xn and w_packed 16-byte aligned, no NULL pointer but logits; everything else is
 * refused before any launch with the outputs untouched. */
int zs_tag_conv(const void* xn, int B, int C, int dtype, const void* w_packed, int N,
                const float* bias, float* frame, int ldf, float* clip, int ldc, float* logits,
                void* stream);

/* ------------------------------------------------------------------ CNN14 (cnns.py:36-78,171-201)
 * zs_conv3x3_bn_relu: NHWC implicit-GEMM conv3x3 pad 1 (no bias) + eval BN + ReLU.
 *   x [B][H][W][Cin] (dtype), w [Cout][3][3][Cin] (dtype), bn folded as scale/shift f32 [Cout]
 *   (y = relu(conv*scale + shift)), out [B][H][W][Cout] (dtype).
 *   k = (ky*3 + kx)*Cin + ci.  Cin == 1 (w rows are the 9 taps zero-padded to 32: [Cout][32]) or
 *   Cin % 32 == 0; any Cout > 0; B, H, W > 0 with B*H*W within an int; non-NULL buffers. */
int zs_conv3x3_bn_relu(const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                       const float* scale, const float* shift, void* out, int dtype, void* stream);
/* zs_avgpool2: 2x2 average pool (floor: an odd last row / column is dropped) NHWC, dtype in/out.
 * B > 0, H >= 2, W >= 2, C > 0, B*H*W within an int; non-NULL buffers. */
int zs_avgpool2(const void* x, int B, int H, int W, int C, void* out, int dtype, void* stream);
/* zs_cnn_head: mean over freq (W) then max + mean over time (H): x [B][H][W][C] -> [B][C] f32.
 * 0 < B <= 65535, H, W, C > 0, B*H*W within an int; non-NULL buffers. */
int zs_cnn_head(const void* x, int B, int H, int W, int C, float* out, int dtype, void* stream);
/* zs_cast: f32 -> dtype element copy (e.g. the bn0'd log-mel as the NHWC C=1 CNN14 input). */
int zs_cast(const float* x, long n, void* y, int dtype, void* stream);

/* ------------------------------------------------------------------ prompt
 * zs_prompt_assemble: dataset/dataset.py:441-453 + utils.py:131-188 on device —
 * sim = emb[b] . labels^T (softmax is monotonic: top-k on sim, ties -> lower index), then
 * ids = head + (label ids + ',')* + tail ("There are l1, l2 in this audio.").
 * label_tok [L][max_tok] int32 with label_len[L]; out hard_ids [B][h_cap] int32 (0-padded,
 * padding_captions utils.py:190-208), hard_len [B], chosen [B][k] int32 (may be NULL). */
int zs_prompt_assemble(const float* emb, int B, int D, const float* labels, int L, int k,
                       const int* label_tok, const int* label_len, int max_tok, int* hard_ids,
                       int h_cap, int* hard_len, int* chosen, void* stream);

/* ------------------------------------------------------------------ mapper / small attention
 * zs_row_attention: per row b, per head h: softmax(scale * q_i . k_j) v_j over j < len[b]
 * (causal: j <= i).  q element (b, i, h, d) at q[(b*L + i)*ldq + h*hd + d], k/v likewise with
 * ldkv, out with ldo (all dtype).  Serves models/mapper.py:49-66 (non-causal, hd 96) and the GPT-2
 * prompt prefill (causal, hd 64).  hd 64 or 96, L <= 256 and 2 * L * hd * 4 bytes of K / V <= 160
 * KiB of LDS (hd 64: L <= 256; hd 96: L <= 213).  Above 64 KiB (L > 128 at hd 64, L > 85 at hd 96)
 * the launch asks for more dynamic LDS than a kernel gets by default; it is served without a
 * hipFuncSetAttribute call (tests/test_gpu_attn_kernels.py runs L = 130 and 256 against float64).
 * Query rows i >= len[b] are written too (causal: over the len[b] keys).  bf16 with hd 64,
 * L <= 32, ldq % 8 == ldkv % 8 == 0 and ldo % 4 == 0 runs the MFMA kernel, which rounds the
 * unnormalised probabilities to bf16 before P.V. */
int zs_row_attention(const void* q, int ldq, const void* k, const void* v, int ldkv, int B, int L,
                     const int* len, int heads, int hd, int causal, float scale, void* out, int ldo,
                     int dtype, void* stream);

/* zs_row_attention_kv: the GPT-2 prompt prefill's attention fused with its KV-cache write
 * (gpt2_prefix_eval.py:99-158 via transformers GPT2Attention with use_cache; replaces the
 * zs_kv_write + zs_row_attention pair of a layer): qkv [B*L][3*heads*64] bf16 (q | k | v, head
 * dim 64), causal over j < len[b], L <= 32; out rows with ldo; k / v of all L rows stored into
 * kc / vc [B*row_stride][heads][Lmax][64] at positions 0..L-1 exactly as zs_kv_write (pos0 NULL)
 * stores them. */
int zs_row_attention_kv(const void* qkv, int B, int L, const int* len, int heads, float scale,
                        void* out, int ldo, void* kc, void* vc, int Lmax, int row_stride,
                        void* stream);

/* zs_cross_attention: nn.MultiheadAttention's core (after in_proj, before out_proj) for short
 * key sets: out(b, i, h) = softmax_j(scale * q(b,i,h) . k(b,j,h)) v(b,j,h), j < Lk; q rows
 * b*Lq + i (ldq), k / v rows b*Lk + j (ldkv), head h at columns h*hd.. (dtype).  Serves the
 * sound-effect cross-attention of ClapCaptionCrossattention[_v2] (models/caption_model.py:100-206,
 * nn.MultiheadAttention(prefix_size, 4)).  Lk <= 64, hd <= 256. */
int zs_cross_attention(const void* q, int ldq, const void* k, const void* v, int ldkv, int B,
                       int Lq, int Lk, int heads, int hd, float scale, void* out, int ldo,
                       int dtype, void* stream);

/* zs_label_topk: sound_effect_choice (caption_model.py:15-20, utils.py:131-137): per row b the
 * k labels (of L, rows of labels [L][D] f32) with the highest similarity emb[b] . label, best
 * first, ties to the lower index (softmax is monotone); idx [B][k] int32 (may be NULL) and the
 * chosen rows gathered into rows [B][k][D] f32.  k <= 16, (D + L) * 4 <= 64 KB. */
int zs_label_topk(const float* emb, int B, int D, const float* labels, int L, int k, int* idx,
                  float* rows, void* stream);

/* ------------------------------------------------------------------ CLAP-guided ("magic") decoding
 * gpt2_prefix_eval.py:341-689 (magic_search, generate_beam_magic and their helpers) batched over C
 * clips, b beams per clip (b = 1: magic_search), W candidates per beam.  Candidate c =
 * (clip*b + beam)*W + w is also the physical row of the GPT-2 KV cache and of the context-hidden
 * store ctx [rows][Lmax][768] that holds its position-pos entries; kvrow [beam][Lmax] names the
 * row holding each position of a beam's history (enlarge/select_past_key_values,
 * gpt2_prefix_eval.py:471-494, as index copies). */

/* zs_bert_embed_ln: HF BertEmbeddings (input_ids, position ids 0..L-1, token type 0) +
 * LayerNorm(eps) for rows = texts*L token rows (ids int32 [rows], row r = text*L + j): x f32
 * [rows][768], and h (hdtype) the same values as the next GEMM's operand (may be NULL).
 * Replaces BertModel's embedding layer under ASE.encode_text (text_encoder.py:64-68). */
int zs_bert_embed_ln(const int* ids, int rows, int L, const float* word, const float* pos,
                     const float* type0, const float* ln_w, const float* ln_b, float eps, float* x,
                     void* h, int hdtype, void* stream);

/* zs_layernorm_dual: LayerNorm of f32 rows y (ldy) into f32 x (ldx) and the operand copy h
 * (hdtype, ldh; may be NULL) -- BERT's post-LN residual stream (BertSelfOutput / BertOutput).
 * C must be 768. */
int zs_layernorm_dual(const float* y, int rows, int C, int ldy, const float* ln_w,
                      const float* ln_b, float eps, float* x, int ldx, void* h, int ldh,
                      int hdtype, void* stream);

/* zs_row_topk: per row of f32 logits [R][V] (row stride ld): the k largest (best first, ties to
 * the lower index) as out_idx [R][k] int32 and out_val [R][k] = log(softmax) (mode 0,
 * ComputeMagicScore gpt2_prefix_eval.py:560-562) or softmax probability (mode 1,
 * PlugAndPlayContrastiveDecodingOneStepFast 411-413).  V <= 51200, k <= 64. */
int zs_row_topk(const float* logits, int R, int V, long ld, int k, int mode, float* out_val,
                int* out_idx, void* stream);

/* zs_magic_expand: candidate c = beam*W + w inherits its beam's history: kvrow_c[c][t] =
 * kvrow[beam][t] for t < pos[beam], pos_c[c] = pos[beam] (enlarge_past_key_values 471-480). */
int zs_magic_expand(const int* kvrow, const int* pos, int nbeams, int W, int Lmax, int* kvrow_c,
                    int* pos_c, void* stream);

/* zs_magic_maxcos: maxcos[c] = max over t < pos[beam] of cos(ctx[kvrow[beam][t]][t], hid[c])
 * (plug_and_play_fast_ranking 514-520, prefix_length 1), hid [ncand][768] = the candidates' ln_f
 * rows (dtype); then stores hid[c] at ctx[c][pos[beam]]. */
int zs_magic_maxcos(const void* hid, int ncand, int W, void* ctx, int Lmax, const int* kvrow,
                    const int* pos, float* maxcos, int dtype, void* stream);

/* zs_magic_score: per clip k, over its first nact*W candidates (nact = 1 at the first beam step):
 * clap = log_softmax_c(cos(text[c], audio[k]) / temp) (gpt2_prefix_eval.py:541-547);
 * score[c] = (1 - alpha) pval[c] - alpha maxcos[c] + beta clap[c] (plug_and_play_fast_ranking
 * 530-531).  text [C*b*W][E], audio [C][E] f32.  b <= 8, W <= 64, nact*W <= 512. */
int zs_magic_score(const float* pval, const float* maxcos, const float* text, const float* audio,
                   int C, int E, int b, int W, int nact, float temp, float alpha, float beta,
                   float* score, void* stream);
/* zs_magic_score_t: zs_magic_score with the score divided by score_temp (> 0):
 * generate_beam_magic's `temperature` (gpt2_prefix_eval.py:629). */
int zs_magic_score_t(const float* pval, const float* maxcos, const float* text, const float* audio,
                     int C, int E, int b, int W, int nact, float temp, float alpha, float beta,
                     float score_temp, float* score, void* stream);

/* zs_magic_step: one selection step per clip (one block each).  greedy = 0: generate_beam_magic
 * 626-683 (first: topk(b) of beam 0's W scores; later: stopped beams keep candidate 0 at zero
 * cost, length-normalised topk over b*W, scores = avg * seq_len); greedy = 1 (b = 1):
 * magic_search's argmax 459-468.  Rewrites each beam's kvrow / token row from its source beam,
 * kvrow[beam][pos] = chosen candidate row, pos += 1, tokens[beam][step] = chosen id, copies the
 * candidate's ln_f row hid[c] to sel_h[beam] (the next LM-head input); a clip is frozen
 * (cdone[k] = 1) once all its beams stopped or step + 1 >= max_steps[k]; ntok[k] = tokens
 * emitted.  tokens [C*b][Smax], kvrow [C*b][Lmax] int32. */
int zs_magic_step(const float* score, const int* cand, int C, int b, int W, int first, int greedy,
                  int stop, int step, const int* max_steps, float* scores, float* seq_len,
                  int* stopped, int* tokens, int Smax, int* kvrow, int Lmax, int* pos, int* cdone,
                  int* ntok, const void* hid, void* sel_h, int dtype, void* stream);

/* ------------------------------------------------------------------ Mistral-7B decoder (C5)
 * predict_mistralai_multilingual.py:97-111 / models/caption_model.py:340-413: batched greedy
 * MistralForCausalLM.generate over inputs_embeds.  head_dim 128, grouped-query attention.
 * Split-K GEMM results are f32 slabs [nsplit][M][N] (split stride ss) summed in order by their
 * consumer (RoPE/KV append, SiLU*up, add+RMSNorm): deterministic, no reduction launch. */

/* zs_fp8_gemm_rows: weight-only fp8 GEMM for M <= 64 rows (decode): out[s][m][n] = scale[n] *
 * sum_{k in split s} A[m][k] W[n][k]; A bf16 [M][lda], W8 the fp8 e4m3 (OCP) codes of W [N][K]
 * TILE-PACKED [K/1024][ceil(N/128)][8][16][64][16 B] (zsaac/mistral.py fp8_pack_tiles: block
 * (s, t, w, j), lane l = W[128 t + 16 w + (l & 15)][1024 s + 64 j + 16 (l >> 4) .. +16], rows past
 * N zero), scale f32 [N] (one per output channel), K % 1024 == 0, splits of 1024 along K
 * (zs_fp8_splits(K) of them), ldo >= N.
 * Replaces the NF4-quantised q/k/v/o/gate/up/down projections of the LoRA-wrapped Mistral
 * (caption_model.py:355-364). */
int zs_fp8_gemm_rows(const void* A, int lda, const void* W8, const float* scale, int M, int N,
                     int K, float* out, long split_stride, int ldo, void* stream);
int zs_fp8_splits(int K);

/* zs_fp8_gemm_run: the same product for M <= 32 with one workgroup per (128-column tile, run of
 * ks consecutive splits, k half of kh), the run summed in registers: out gets
 * zs_fp8_splits(K) / ks * kh slabs (slab (run, half) at index run * kh + half; kh 2 halves each
 * split between two workgroups, for short streams).
 * act != NULL (GLU; ks == zs_fp8_splits(K)): W is the gate|up matrix with rows glu-interleaved
 * (zsaac/mistral.py glu_interleave) and act[m][f] = silu(gate_f) * up_f is written directly as
 * bf16 [M][ld_act] (N / 2 columns; out unused) -- MistralMLP's act_fn(gate_proj(x)) * up_proj(x)
 * (transformers MistralMLP, called from caption_model.py:355-364's generate). */
int zs_fp8_gemm_run(const void* A, int lda, const void* W8, const float* scale, int M, int N,
                    int K, int ks, int kh, float* out, long split_stride, int ldo, void* act,
                    int ld_act, const float* rss, int nch, float eps, void* stream);

/* zs_mistral_add_ss: the decode form of zs_mistral_add_rmsnorm when the next GEMM applies the
 * norm (zs_fp8_gemm_run with rss; MistralRMSNorm's weight folded into that GEMM): x[m] +=
 * sum_s y[s][m] (y may be NULL), xb[m] = bf16(x[m]) and rss[c][m] (row stride 32) = sum of x^2 over
 * columns 512 c .. 512 c + 511; M <= 32, D % 512 == 0.  zs_fp8_gemm_run(..., rss, D / 512 <= 8, eps)
 * then scales output row m by rsqrt(sum_c rss[c][m] / K + eps). */
int zs_mistral_add_ss(float* x, const float* y, int nsplit, long ss, int M, int D, void* xb,
                      float* rss, void* stream);

/* zs_mistral_embed: prefill rows b*P + i (P = H + ns + nt): embed[hard[b][i]] (i < H, pads
 * included as the reference attends them), soft[b][i-H] (ns rows, f32), embed[tail[i-H-ns]]
 * (the language tag); or, with tok != NULL, decode rows embed[tok[m]].  x f32 [M][D]. */
int zs_mistral_embed(const int* hard, int H, const float* soft, int ns, const int* tail, int nt,
                     const int* tok, const void* emb, int D, int M, float* x, int dtype,
                     void* stream);

/* zs_mistral_add_rmsnorm: x[m] += sum_s y[s][m] (y may be NULL), h[m] = w * (x[m] *
 * rsqrt(mean(x[m]^2) + eps)) (MistralRMSNorm; w NULL = folded into the next GEMM).  x f32 [M][D]
 * updated in place (untouched when y is NULL), h [M][D] in hdtype; D % 4 == 0, D <= 16384,
 * ss % 4 == 0, x / y / h 16-byte aligned (checked). */
int zs_mistral_add_rmsnorm(float* x, const float* y, int nsplit, long ss, int M, int D, float eps,
                           const float* w, void* h, int hdtype, void* stream);

/* zs_mistral_rope_kv: q|k|v slabs [nsplit][M][(H + 2 KVH) * 128] -> rotary-embedded q [M][H*128]
 * and k, plus v, appended to the caches [seq][KVH][Lmax][128] at position pos[m] (seq =
 * m / rows_per_seq); cos / sin [Lmax][64] f32 tables (HF rotary, rotate_half).  Element-wise
 * accesses: no alignment requirement beyond the element type, any ss.  The caller guarantees
 * 0 <= pos[m] < Lmax and caches of ceil(M / rows_per_seq) sequences (pos is device memory: not
 * checked); only rows pos[m] of the caches are written. */
int zs_mistral_rope_kv(const float* qkv, int nsplit, long ss, int M, int H, int KVH,
                       const int* pos, int rows_per_seq, const float* cosb, const float* sinb,
                       void* q, void* kc, void* vc, int Lmax, int dtype, void* stream);

/* zs_fp8_unpack_bf16: the tile-packed fp8 codes of W [N][K] (see zs_fp8_gemm_rows) -> row-major
 * bf16 W-codes [N][K] (exact; the per-channel scale is not applied).  zs_scale_cols:
 * x[m][n] *= scale[n] for an f32 [M][ld] matrix.  Together with zs_gemm they run a prefill's
 * M > 64 rows as one tiled MFMA GEMM (weights read once, not once per 64 rows). */
int zs_fp8_unpack_bf16(const void* W8, int N, int K, void* out, void* stream);
int zs_scale_cols(float* x, int M, int N, int ld, const float* scale, void* stream);

/* zs_mistral_silu_mul: act[m][f] = silu(gate) * up from gate|up slabs [nsplit][M][2F] whose
 * columns are glu-interleaved: gate f at 16 (f / 8) + 8 (f / 4 % 2) + f % 4, up f at that + 4.
 * act [M][F] dense in dtype; F % 8 == 0 (so the M F / 4 four-column items are exact), ss % 4 == 0,
 * gu and act 16-byte aligned (checked). */
int zs_mistral_silu_mul(const float* gu, int nsplit, long ss, int M, int F, void* act, int dtype,
                        void* stream);

/* zs_mistral_attention: causal GQA attention, query row m against keys 0..pos[m] of sequence
 * m / rows_per_seq, kv head h / (H / KVH), softmax((q k^T) / sqrt(128)) v -> out [M][H*128]. */
int zs_mistral_attention(const void* q, int M, int H, int KVH, const int* pos, int rows_per_seq,
                         const void* kc, const void* vc, int Lmax, void* out, int dtype,
                         void* stream);

/* zs_mistral_decode_attention: one decode step (row m = sequence m, new position pos[m]):
 * zs_mistral_rope_kv + zs_mistral_attention (rows_per_seq 1) in one launch -- q / k / v summed
 * from the slabs and rotated in registers, k / v row pos[m] appended to the caches, keys
 * 0..pos[m]-1 read from them and key pos[m] from registers. */
int zs_mistral_decode_attention(const float* qkv, int nsplit, long ss, int M, int H, int KVH,
                                const int* pos, const float* cosb, const float* sinb, void* kc,
                                void* vc, int Lmax, void* out, int dtype, void* stream);

/* ------------------------------------------------------------------ GPT-2 decode
 * zs_gpt2_prefill_embed: clap_to_gpt (caption_model.py:315-329) + the caller's wte lookup
 * (predict_prompt.py:133) + GPT-2 input embedding:  row b, position p < P_b = hard_len[b]+n_soft:
 *   e = p < H_b ? wte[hard_ids[b][p]] : soft[b][p-H_b]   (prefix_embed, written to `embed`)
 *   x = e + wpe[p]                                         (transformer input, written to `x`)
 * rows padded to Pmax with zeros.  plen[b] = P_b, last_row[b] = b*Pmax + P_b - 1.  wte/wpe in
 * dtype, soft f32 with clip b's n_soft*D prefix at soft + b*soft_ld. */
int zs_gpt2_prefill_embed(const int* hard_ids, const int* hard_len, int h_cap, const float* soft,
                          int soft_ld, int n_soft, const void* wte, const void* wpe, int B,
                          int Pmax, int D, float* embed, float* x, int* plen, int* last_row,
                          int dtype, void* stream);

/* zs_kv_write: copy k,v of `n` tokens per row from qkv [R*n][3D] into the cache
 * kc/vc [rows][heads][Lmax][hd] at cache row r*row_stride, positions pos0[r] + i (pos0 NULL -> 0).
 * row_stride = beam puts a clip's beam-search prompt in its first beam row. */
int zs_kv_write(const void* qkv, int R, int n, int D, int heads, const int* pos0, int row_stride,
                void* kc, void* vc, int Lmax, int dtype, void* stream);

/* zs_decode_attention: one new token per row r at position pos[r]: append its k,v (from
 * qkv[r]) to the cache, attend over positions 0..pos[r] (kv row for position j of row r is
 * kvrow[r*Lmax + j] when kvrow != NULL, else r — the beam-search history indirection),
 * scale 1/sqrt(hd), f32 softmax.  out [R][D] (dtype).  HF GPT2Attention eager semantics. */
int zs_decode_attention(const void* qkv, int R, int D, int heads, void* kc, void* vc, int Lmax,
                        const int* pos, const int* kvrow, void* out, int dtype, void* stream);

/* zs_decode_attention_map: zs_decode_attention over a compacted row set (bf16, no kvrow):
 * qkv/out rows are compact slots c in [0, R); the physical decode row of slot c is rowmap[c]
 * (the cache is indexed physically).  The position of slot c is cpos[c] when cpos != NULL (as
 * written by zs_embed_tokens_map), else pos[rowmap[c]].  rowmap[c] >= nphys marks a padding
 * slot: its out row is zeroed and the cache is untouched. */
int zs_decode_attention_map(const void* qkv, int R, const int* rowmap, int nphys, int D, int heads,
                            void* kc, void* vc, int Lmax, const int* pos, const int* cpos,
                            void* out, int dtype, void* stream);

/* zs_embed_tokens: x[r] = wte[tok[r]] + wpe[pos[r]] (f32 out), optional row gather. */
int zs_embed_tokens(const int* tok, const int* pos, const void* wte, const void* wpe, int R, int D,
                    float* x, int dtype, void* stream);

/* zs_embed_tokens_map: x[c] = wte[tok[rowmap[c]]] + wpe[pos[rowmap[c]]] for compact slots
 * c in [0, R); padding slots (rowmap[c] >= nphys) get x[c] = 0.  cpos (optional, [R]) receives
 * pos[rowmap[c]] (0 for padding) for zs_decode_attention_map. */
int zs_embed_tokens_map(const int* tok, const int* pos, const int* rowmap, int nphys,
                        const void* wte, const void* wpe, int R, int D, float* x, int* cpos,
                        int dtype, void* stream);

/* zs_compact_rows: stable compaction of the rows still decoding.  rowmap[0..n) = the r with
 * done[r] == 0 in increasing order, rowmap[n..nrows) = nrows (padding), *n_active = n.
 * Lets a greedy decode skip the rows that already emitted a stop token (the reference keeps
 * computing them, gpt2_prefix_eval.py:200-215; their outputs are discarded either way). */
int zs_compact_rows(const int* done, int nrows, int* rowmap, int* n_active, void* stream);

/* zs_lmhead_topk: per row m of A [M][lda] (dtype) against W [V][K] (dtype, contiguous rows; tied
 *   wte): logits = A W^T, split in column blocks of 128; per (row, block) writes the block's max,
 *   sum(exp(logit - max)) and its top-`topk` (value, index), ordered by value descending, then
 *   index ascending (ties -> lower index, in the list and at its cut).
 *   part_stat [M][nblk][2] f32, part_val [M][nblk][topk] f32, part_idx [M][nblk][topk] int32,
 *   nblk = ceil(V/128); every (row, block) is written.  A last block with fewer than topk
 *   columns fills its list with padding entries (value -inf, index 0x7fffffff).  1 <= topk <= 8.
 *   part_stat may be NULL (argmax callers: greedy generate2, get_prefix_tokens): the max /
 *   sum-exp pass is then skipped and nothing is written there.  With row_norm != 0 each A row is
 *   L2-normalised first (logits / max(||a||, 1e-12))
 *   (get_prefix_tokens, gpt2_prefix_eval.py:271-278: W must then be normalize(wte)).
 *   Accepts: M, K, V > 0, K % 32 == 0, lda % 8 == 0 and lda >= K (padding columns are not read),
 *   A and W 16-byte aligned, dtype ZS_F32 / ZS_BF16; everything else is refused before a launch. */
int zs_lmhead_topk(int M, int K, int V, int dtype, const void* A, int lda, const void* W,
                   int topk, int row_norm, float* part_stat, float* part_val, int* part_idx,
                   void* stream);
/* zs_lmhead_topk_t: zs_lmhead_topk on logits / temperature (temperature > 0; row_norm needs 1):
 * generate2 / generate_beam's `temperature` (gpt2_prefix_eval.py:121, 196). */
int zs_lmhead_topk_t(int M, int K, int V, int dtype, const void* A, int lda, const void* W,
                     int topk, int row_norm, float temperature, float* part_stat, float* part_val,
                     int* part_idx, void* stream);
int zs_lmhead_nblk(int V);

/* zs_argmax_finalize: merge zs_lmhead_topk partials (topk 1) into idx[M] (lower index on ties). */
int zs_argmax_finalize(const float* part_val, const int* part_idx, int M, int nblk, int* idx,
                       void* stream);

/* ------------------------------------------------------------------ teacher-forced scoring
 * log p(caption | clip): the cross-entropy the reference trains on (train_prompt.py:133, over
 * ClapCaption_prompt.forward's logits, caption_model.py:297-313), on the sequence generate2 /
 * generate_beam condition on (predict_prompt.py:129-148), temperature 1.
 *
 * zs_gpt2_score_embed: zs_gpt2_prefill_embed's scoring twin.  Clip b, H_b = hard_len[b],
 * n = n_soft, T_b = cap_len[b], cap = cap_ids [B][Tmax]:
 *   row b of x [B][Smax][D] = [wte(hard[b][:H_b]) ; soft[b] ; wte(cap[b][:T_b-1])] + wpe, zeros
 *   from S_b = H_b + n + max(T_b - 1, 0) on;  plen[b] = S_b;
 *   score_rows [B][Tmax] = b*Smax + H_b + n - 1 + t  (the row that predicts cap[b][t]) for
 *   t < T_b, b*Smax beyond;  tgt [B][Tmax] = cap[b][t] for t < T_b, -1 beyond.
 * Smax >= h_cap + n_soft + Tmax - 1, n_soft >= 1.  Nothing is clamped silently: an id outside
 * [0, V) is embedded as id 0 and, if a caption id, its target becomes -1; a length outside
 * [0, h_cap] / [0, Tmax] is cut to it; the number of such ids and lengths is ADDED to status[0]
 * (the caller zeroes it before and raises on a count). */
int zs_gpt2_score_embed(const int* hard_ids, const int* hard_len, int h_cap, const float* soft,
                        int soft_ld, int n_soft, const int* cap_ids, const int* cap_len, int Tmax,
                        const void* wte, const void* wpe, int V, int B, int Smax, int D, float* x,
                        int* plen, int* score_rows, int* tgt, int* status, int dtype,
                        void* stream);

/* zs_lmhead_nll: the LM head of scoring (lm_logits = hidden . wte^T, caption_model.py:297-313, then
 * the cross-entropy of train_prompt.py:133), fused: per row m of A [M][K] against W [V][K] and per
 * column block of 128, the block's max and sum(exp(logit - max)) (part_stat [M][nblk][2], the
 * layout and arithmetic of zs_lmhead_topk) and its top-1 (part_val / part_idx [M][nblk], ties ->
 * lower index); and tgt_logit[m] = logit[m][tgt[m]], written by the one block that holds that
 * column (no atomics).  A row with tgt[m] outside [0, V) writes no target logit.  No top-k list
 * and no [M][V] logits are written.  K % 32 == 0, lda % 8 == 0, A and W 16-byte aligned. */
int zs_lmhead_nll(int M, int K, int V, int dtype, const void* A, int lda, const void* W,
                  const int* tgt, float* part_stat, float* part_val, int* part_idx,
                  float* tgt_logit, void* stream);

/* zs_nll_finalize: merges zs_lmhead_nll's partials, M = B x Tmax rows (caption b's rows are
 * b*Tmax .. b*Tmax + Tmax - 1).  Per row: lse = log sum exp(logit), argmax[m] (lower index on
 * ties), logprob[m] = tgt_logit[m] - lse -- log_softmax(logits)[target], the summand of the
 * cross-entropy (train_prompt.py:133) -- or 0 for a row whose tgt is outside [0, V).  Per
 * caption: sum[b] = its rows' logprob added in position order, cnt[b] = its rows with a target.
 * lse may be NULL.  Every reduction runs in a fixed order: results are bit-identical from run to
 * run. */
int zs_nll_finalize(const float* part_stat, const float* part_val, const int* part_idx,
                    const int* tgt, const float* tgt_logit, int M, int nblk, int V, int B,
                    int Tmax, float* logprob, float* lse, int* argmax, float* sum, int* cnt,
                    void* stream);

/* ------------------------------------------------------------------ retrieval metrics
 * zs_sim_rank: the rank of given gallery items, the quantity behind a2t / t2a
 * (retrieval/tools/utils.py:169-251: `np.argsort(d)[::-1]` over a materialised similarity row,
 * then `np.where(inds == i)`), fused.  Queries Q [M][ldq], gallery G [N][ldg] (dtype),
 * sim[m][n] = Q[m] . G[n] accumulated in f32; targets tgt [M][T] int32, 1 <= T <= 8.  For every
 * (m, t) with j = tgt[m][t] in [0, N):
 *   tgt_sim[m][t] = sim[m][j]
 *   rank[m][t]    = #{n != j : sim[m][n] > sim[m][j]} + #{n < j : sim[m][n] == sim[m][j]}
 * -- the 0-based position of j in the row sorted by value descending, then index ascending.  A
 * target outside [0, N) gives rank -1 and tgt_sim 0; two targets of a row may name one column.
 * No [M][N] matrix and no per-block partials exist anywhere: the kernel runs twice (first the
 * blocks that hold a target store its similarity, then every block counts), so the target's value
 * and the values compared with it come from the same MFMA chain and exact duplicates tie; counts
 * are integer atomics on rank (zeroed here, on `stream`), hence independent of the block order
 * and bit-identical from run to run.
 * Accepts: M, N, K > 0, K % 32 == 0, ldq / ldg % 8 == 0 and >= K (padding columns are not read),
 * Q and G 16-byte aligned, no NULL pointer, M x T < 2^31; everything else is refused before any
 * launch with the outputs untouched. */
int zs_sim_rank(int M, int N, int K, int dtype, const void* Q, int ldq, const void* G, int ldg,
                const int* tgt, int T, float* tgt_sim, int* rank, void* stream);

/* zs_sim_topk_finalize: nearest neighbours (`cosine_similarity(...).topk(5)`,
 * data_handing/embeddings_related_generator.py:19-28; `audio_emb @ text_embeds.t()` then the best
 * class, retrieval/zero_shot_classification.py:82-106): merges the [M][nblk][kpart] partial lists
 * zs_lmhead_topk writes (W = the gallery) into the row's global top-k, out_val / out_idx [M][k],
 * value descending, then index ascending; padding entries (-inf, 0x7fffffff) come last.
 * 1 <= k <= kpart <= 8.  One wave per row, fixed order. */
int zs_sim_topk_finalize(const float* part_val, const int* part_idx, int M, int nblk, int kpart,
                         int k, float* out_val, int* out_idx, void* stream);

/* ------------------------------------------------------------------ text memory bank
 * map2memory (predict_prompt.py:23-29): an embedding is replaced by the softmax-weighted mix of a
 * bank of caption embeddings, `softmax(100 * q @ T.T) @ T`, normalised.  Queries Q [M][ldq], bank
 * [N][ldb] (dtype f32 or bf16, rows as stored), float scale:
 *   z[m][n] = scale * (Q[m] . bank[n])           dots accumulated in f32
 *   lse[m]  = log sum_n exp(z[m][n])
 *   mix[m]  = sum_n exp(z[m][n] - lse[m]) bank[n]                      f32 [M][K]
 * One streaming pass with an online softmax: no [M][N] array exists, every bank tile is fetched
 * once and serves both products.  bf16: bf16 MFMA, f32 accumulation, the softmax weights rounded
 * to bf16 for the second product and the running sum adding the rounded values; f32: exact f32
 * products (v_mfma_f32_32x32x2_f32).  No atomics; a row's result does not depend on M or on the
 * rows that share the launch, and is bit-identical from run to run.
 *
 * zs_memory_nsplit (predict_prompt.py:23-29): the default number of bank splits, a function of
 *   (N, K, dtype) only; -1 for arguments zs_memory_project refuses. */
int zs_memory_nsplit(int N, int K, int dtype);

/* zs_memory_project (predict_prompt.py:23-29): the bank rows are cut into nsplit contiguous
 *   splits (flash-decoding); split s writes, per row m, part_mix[m][s][0..K) = a =
 *   sum_n exp(z - m_s) bank[n], and part_ml[m][s] = (m_s, l_s) = (max z, sum exp(z - m_s)) over
 *   its rows; a split with no rows (nsplit larger than the number of tiles) writes (0, -inf, 0).
 *   part_mix [M][nsplit][K] f32, part_ml [M][nsplit][2] f32.
 *   Accepts: M, N > 0; K % 32 == 0, 32 <= K <= 1024; ldq / ldb % 8 == 0 and >= K (padding
 *   columns are never read); 1 <= nsplit <= 4096; Q, bank, part_mix 16-byte aligned; no NULL.
 *   Everything else is refused (-1 and a message) before any launch, outputs untouched. */
int zs_memory_project(int M, int N, int K, int dtype, const void* Q, int ldq, const void* bank,
                      int ldb, float scale, int nsplit, float* part_mix, float* part_ml,
                      void* stream);

/* zs_memory_merge (predict_prompt.py:23-29): merges the partials in split order:
 *   m* = max_s m_s, L = sum_s l_s e^(m_s - m*), mix = sum_s a_s e^(m_s - m*) / L,
 *   lse = m* + log L; an empty split (0, -inf, 0) contributes nothing (no NaN).
 *   normalize != 0: out[m] = mix[m] / max(||mix[m]||, 1e-12) (the eps convention of
 *   zs_l2norm_rows; the reference divides by the bare norm), else out[m] = mix[m].
 *   out [M][ldo] f32, lse [M] f32 or NULL.  A finished chunk re-enters a later merge as
 *   (mix, lse, 1): banks larger than one tensor, or sharded, are combined this way.
 *   Accepts: M > 0, 1 <= nsplit <= 4096, K as above, ldo % 8 == 0 and >= K, part_mix and out
 *   16-byte aligned, no NULL except lse; everything else is refused before the launch. */
int zs_memory_merge(const float* part_mix, const float* part_ml, int M, int nsplit, int K,
                    int normalize, float* out, int ldo, float* lse, void* stream);

/* zs_prefix_ids_assemble: get_prefix_tokens (gpt2_prefix_eval.py:271-278) with the argmax run
 * only over the soft-prompt rows: out[b][p] = hard_ids[b][p] for p < hard_len[b] (a hard row is
 * wte[id] and its own cosine is the maximum — the caller verifies that every possible hard id
 * beats every other vocabulary row by a margin before taking this path), soft_idx[b][p - H_b]
 * for the n_soft rows after it, 0 for padding rows (zero embeddings: all cosines 0).
 * hard_ids [B][h_cap], soft_idx [B][n_soft], out [B][Pmax] int32. */
int zs_prefix_ids_assemble(const int* hard_ids, int h_cap, const int* hard_len, const int* soft_idx,
                           int n_soft, int B, int Pmax, int* out, void* stream);

/* zs_greedy_step: generate2's per-step bookkeeping (gpt2_prefix_eval.py:208-215) for R rows:
 * tok = argmax(partials); rows already done keep emitting nothing; out_ids[r][step] = tok,
 * out_len[r] = step+1 while not done; done |= tok in {stop0, stop1}; pos[r] += 1 (next position);
 * next_tok[r] = tok.  `step` is read from *step_ctr (device) and *step_ctr += 1 by the last
 * block, so a captured graph replays without host arguments.  all_done[0] = AND(done);
 * all_done[1] is the blocks' arrival counter: zero it once before the first call (every call
 * re-arms it); all_done[2] = the number of rows not done after this step. */
int zs_greedy_step(const float* part_val, const int* part_idx, int R, int nblk, int* step_ctr,
                   int max_steps, int stop0, int stop1, int* out_ids, int* out_len, int* done,
                   int* pos, int* next_tok, int* all_done, void* stream);

/* zs_greedy_init: generate2's state before step 0 (gpt2_prefix_eval.py:186-196) for R rows:
 * pos[r] = plen[r] - 1 (the last prompt position), done = out_len = 0, out_ids[r][0..max_steps)
 * = 0, *step_ctr = 0, all_done[0..2] = 0 -- what zs_greedy_step expects before its first call. */
int zs_greedy_init(int R, const int* plen, int* pos, int* done, int* out_len, int* out_ids,
                   int max_steps, int* step_ctr, int* all_done, void* stream);

/* zs_greedy_step_map: zs_greedy_step where partial row c belongs to physical row rowmap[c]
 * (out_ids, out_len, done, pos, next_tok are physical); padding slots are skipped. */
int zs_greedy_step_map(const float* part_val, const int* part_idx, int R, const int* rowmap,
                       int nphys, int nblk, int* step_ctr, int max_steps, int stop0, int stop1,
                       int* out_ids, int* out_len, int* done, int* pos, int* next_tok,
                       int* all_done, void* stream);

/* zs_sample_rows: one sampled token per row of f32 logits [R][ld] (generate2's `top_p` /
 * `temperature`, gpt2_prefix_eval.py:161-222; the nucleus rule of its lines 197-206), in HF's
 * processor order:
 *   z = logits / temperature;
 *   top_k > 0: keep the min(top_k, V) largest z, ties at the cut to the lower id; probabilities
 *     from here on are renormalised over what is kept;
 *   top_p < 1: order the kept tokens by p descending (ties: lower id first) and keep rank i iff
 *     the mass strictly before it is <= top_p (rank 0 always);
 *   draw: in increasing id order, the first kept token whose running kept mass exceeds
 *     u * kept mass, u = (w + 0.5) * 2^-32, w = the first output word of Philox4x32-10 with the
 *     64-bit `seed` as key and the counter (row_id[r], *step_ctr, 0, 0) -- row_id NULL: r.  The
 *     step is read on the device (as zs_greedy_step reads it, which then advances it), and a
 *     row's draw depends on its id, not on its slot in the launch.
 * part_val[r] = logits[r][tok], part_idx[r] = tok: the [R][1][1] partials of an nblk = 1 argmax,
 * so zs_greedy_step / zs_greedy_step_map (nblk = 1) do the stop / length / done bookkeeping.
 * logprob[r] (optional) = log softmax(logits[r])[tok] at temperature 1, unfiltered (what
 * zs_nll_finalize sums for a caption); kept[r] (optional, [R][2]) = (number of tokens kept, their
 * share of softmax(z)).  One workgroup per row, the row read once into registers; no sort, no
 * atomics: the same inputs give the same bits.  A row that is -inf everywhere is not meaningful
 * (the last token is returned).
 * Accepts: R > 0, 1 <= V <= 65536, ld >= V, temperature > 0, top_p > 0 (>= 1: off), top_k >= 0
 * (0 or >= V: off), pointers 4-byte aligned (rows that all start on 16 bytes are read as float4);
 * everything else is refused before a launch. */
int zs_sample_rows(const float* logits, int R, int V, int ld, const int* row_id,
                   const int* step_ctr, long seed, float temperature, int top_k, float top_p,
                   float* part_val, int* part_idx, float* logprob, float* kept, void* stream);

/* zs_gpt2_decode_persist: every remaining step of generate2 (gpt2_prefix_eval.py:161-222: the
 * 67-step loop of model.gpt(inputs_embeds=...) -> argmax -> stop check) for ONE batch of R <= 64
 * rows (the reference's eval batch), bf16, as one persistent launch of `grid` (48, 96 or 192)
 * 256-thread workgroups (half a CU each; the caller keeps the concurrent launches' grids
 * co-resident): per step the 12 GPT2Blocks (ln_1 affine folded into c_attn and ln_2's into c_fc),
 * ln_f, the tied LM head with its argmax (ties -> lower id) and zs_greedy_step's bookkeeping,
 * until every row stopped or max_steps.  Starts from the state zs_greedy_step left after step 0
 * (next_tok, pos, done, out_ids, out_len, *step_ctr, all_done[0]) and commits that state after
 * every step.  layer_w: 12 x 8 device pointers {c_attn W, its bias, attn.c_proj W, bias, c_fc W,
 * its bias, mlp.c_proj W, bias}, each W (= Conv1D weight transposed, [N][K] bf16; c_attn's with
 * ln_1's weight folded in, c_fc's with ln_2's) in MFMA fragment order [N/16][K/32][64][8] (block j,
 * k-step s, lane l = W[16 j + l % 16][32 s + 8 (l / 16) .. + 8]); the c_attn and c_fc biases are f32
 * [2][N]: row 0 the bias with the LayerNorm's beta folded in (b + beta W), row 1 the folded
 * weight's column sums cs[n] = sum_k W'[n][k] -- the LayerNorm runs in the GEMM epilogue as
 * rstd (x W' - mean cs) + b'; the projections' biases are f32 [N].  wte_packed: the tied LM head
 * with ln_f's weight folded in, bf16(g o wte[v]), in the same order, [ceil(V/16)][24][64][8] (rows
 * past V zero); lm_bias f32 [2][ceil(V/16) 16]: beta . wte[v] (ln_f's bias through the head), then
 * the column sums of the folded head; logit[v] = LN(x) . (g o wte[v]) + lm_bias[0][v];
 * temperature > 0 divides the logits before the argmax (gpt2_prefix_eval.py:196);
 * kv: 24 pointers {kc[0..11], vc[0..11]}, each [R][12][Lmax][64] bf16 (zs_kv_write layout),
 * 128-byte aligned.  ws: scratch of zs_decode_persist_workspace_bytes() bytes, 256-byte aligned,
 * private to one launch in flight.  exclusive != 0: each workgroup also requests LDS past half a
 * CU, so no two exclusive workgroups share a CU (the dispatcher otherwise doubles workgroups up
 * while CUs idle); the caller keeps the exclusive workgroups in flight <= the CU count.  Every
 * output element is computed by the same operations
 * whatever `grid` (each GEMM element: four K-quarter MFMA chains summed (p0 + p1) + (p2 + p3);
 * LayerNorm statistics (one pass, sum x and sum x^2), attention and argmax in fixed orders), so ids and state do not depend on the grid
 * and equal zs_gpt2_decode_phases'.  A grid that cannot become co-resident gives up after a
 * bounded wait: all_done[1] = -1, zs_decode_persist_status reports timed_out != 0, and the state
 * in memory is the last committed step's (resume with zs_gpt2_decode_phases). */
int zs_decode_persist_workspace_bytes(void);
int zs_gpt2_decode_persist(int R, int Lmax, int max_steps, int stop0, int stop1, int V,
                           const void* wte, const void* wpe, const void* wte_packed,
                           float temperature, const void* const* layer_w,
                           const float* lm_bias, void* const* kv, int* pos,
                           int* next_tok, int* done, int* out_ids, int* out_len, int* step_ctr,
                           int* all_done, void* ws, long ws_bytes, int grid, int exclusive,
                           void* stream);
/* zs_gpt2_decode_phases: `steps` decode steps of the same computation as separate launches (one
 * per phase of every block, the LM head and the bookkeeping: 62 per step; each a no-op once
 * all_done[0] is set, so a graph-captured chunk can run past the end) -- the per-step path of
 * zs_gpt2_decode_persist (no co-residency needed; the give-up fallback), bit-identical to it.
 * Launch i of a step: 5 l + {0 A, 1 B, 2 C, 3 D, 4 E} for block l, 60 = F (ln_f + LM head), 61 =
 * the bookkeeping.  zs_tune_set("dg_win_lo", a) / ("dg_win_hi", b) (defaults 0 / 62, 0 <= a <= 61,
 * 1 <= b <= 62) narrow a call, of this entry and of zs_gpt2_decode_phases_f32, to the launches
 * a <= i < b: then steps must be 1, and an empty window (a >= b) fails with ZS_ERR_ARG.  Every call
 * still zeroes the workspace's first 4096 bytes (barrier words and the argmax keys F raises), and
 * every phase hands its output on through memory, so a test can run one phase on inputs it wrote
 * (tests/test_gpu_grid_kernels.py); C and E update x in place: once per workspace contents. */
int zs_gpt2_decode_phases(int R, int Lmax, int max_steps, int stop0, int stop1, int V,
                          const void* wte, const void* wpe, const void* wte_packed,
                          float temperature, const void* const* layer_w,
                          const float* lm_bias, void* const* kv, int* pos,
                          int* next_tok, int* done, int* out_ids, int* out_len, int* step_ctr,
                          int* all_done, void* ws, long ws_bytes, int steps, int grid,
                          void* stream);
/* zs_gpt2_decode_persist_f32 / zs_gpt2_decode_phases_f32: the same decode in f32 (the parity
 * mode; replaces the same generate2 loop, gpt2_prefix_eval.py:161-222, in fp32): wte / wpe f32
 * [V][768] / [1024][768]; layer_w 12 x 8 pointers in the same order, each W f32 in 16-k fragment
 * order [N/16][K/16][64][4] (block j, k-step s, lane l = W[16 j + l % 16][16 s + 4 (l / 16) .. + 4]),
 * c_attn's / c_fc's with the LayerNorm's weight folded in (W diag(g), f32) and biases f32 [N]
 * (b + W beta); wte_packed f32 g o wte[v] (ln_f's weight) in that order [ceil(V/16)][48][64][4];
 * lm_bias f32 [ceil(V/16) 16] (beta . wte[v]); kv f32 [R][12][Lmax][64]; ws of
 * zs_decode_persist_f32_workspace_bytes().  The LayerNorms are two-pass (mean, then squared
 * deviations) and normalise rows in registers before exact-f32 MFMAs (v_mfma_f32_16x16x4_f32);
 * grid 192 only.  The persistent and phase forms give identical ids, as the bf16 pair. */
int zs_decode_persist_f32_workspace_bytes(void);
int zs_gpt2_decode_persist_f32(int R, int Lmax, int max_steps, int stop0, int stop1, int V,
                               const void* wte, const void* wpe, const void* wte_packed,
                               float temperature, const void* const* layer_w,
                               const float* lm_bias, void* const* kv, int* pos,
                               int* next_tok, int* done, int* out_ids, int* out_len, int* step_ctr,
                               int* all_done, void* ws, long ws_bytes, int grid, int exclusive,
                               void* stream);
int zs_gpt2_decode_phases_f32(int R, int Lmax, int max_steps, int stop0, int stop1, int V,
                              const void* wte, const void* wpe, const void* wte_packed,
                              float temperature, const void* const* layer_w,
                              const float* lm_bias, void* const* kv, int* pos,
                              int* next_tok, int* done, int* out_ids, int* out_len, int* step_ctr,
                              int* all_done, void* ws, long ws_bytes, int steps, int grid,
                              void* stream);
int zs_decode_persist_status(const void* ws, int* timed_out);
/* zs_decode_persist_set_stamps: diagnostic phase timing (tools/persist_stamps.py): with buf !=
 * NULL ([grid][128] u64), thread 0 of every workgroup of later launches writes s_memrealtime
 * (100 MHz) at each barrier arrive (slot 2i) / wait end (2i + 1) of decode step `step`, and at
 * that step's start (127) / end (126); ws != NULL: only the launches on that workspace (one of
 * several concurrent grids).  buf NULL turns it off. */
int zs_decode_persist_set_stamps(void* buf, int step, const void* ws);

/* zs_beam_step: generate_beam's per-step update (gpt2_prefix_eval.py:119-151) for C clips x
 * `beam` rows, from zs_lmhead_topk partials (topk >= beam) with log(softmax) semantics.
 * first != 0: step 0 (row c*beam of each clip is the only live source).  Updates scores,
 * seq_len, stopped, the token history tokens [R][max_steps], the kv-row indirection table
 * kvrow [R][Lmax] (history of the chosen source row + this step's own slot), pos[R],
 * next_tok[R]; all_done[0] = every row stopped. */
int zs_beam_step(const float* part_stat, const float* part_val, const int* part_idx, int C,
                 int beam, int nblk, int topk, int first, int stop, int* step_ctr, int max_steps,
                 float* scores, float* seq_len, int* stopped, int* tokens, int* tokens_tmp,
                 int* kvrow, int* kvrow_tmp, int Lmax, int* pos, int* next_tok, int* all_done,
                 void* stream);

/* ------------------------------------------------------------------ training the MLP mapper
 * The backward pass behind the teacher-forced cross-entropy (train_prompt.py:133 over
 * ClapCaption_prompt.forward, caption_model.py:297-313) with GPT-2 frozen, AdamW and the
 * training-side noise.  Every matrix product of the backward pass is zs_gemm on
 * a transposed operand (zs_transpose_cast); the entries below are what is not a GEMM.  None uses
 * an atomic; every reduction runs in a fixed order (bit-identical results from run to run).
 *
 * zs_attention_bwd: the backward of GPT2Attention's causal softmax(Q K^T / 8) V (transformers,
 * reached from caption_model.py:308) on the packed qkv [B*L][3*heads*64] the forward reads, given
 * d_out [B*L][heads*64]:  P = softmax(Q K^T / 8) over j <= i recomputed per (b, head),
 * dP = dO V^T, D_i = sum_j P_ij dP_ij (= dO_i . O_i), dV = P^T dO, dS = P o (dP - D),
 * dQ = dS K / 8, dK = dS^T Q / 8, into dqkv in qkv's packing (all dtype, f32 arithmetic).  Rows
 * i >= len[b] (len NULL: L) are ignored as queries and as keys, are never read, and get zeros.
 * Head dim 64, 1 <= L <= 256; the three buffers 16-byte aligned, dqkv distinct from the inputs. */
int zs_attention_bwd(const void* qkv, const void* d_out, int B, int L, const int* len, int heads,
                     void* dqkv, int dtype, void* stream);

/* zs_layernorm_bwd: dx of y = LayerNorm(x) g + b (GPT-2 ln_1 / ln_2 / ln_f) from x and dy:
 * a = dy o g (g NULL: 1), dx = rstd (a - mean(a) - xhat mean(a o xhat)) + res (res NULL: 0; res
 * may be dx).  rows != NULL (ln_f of the scored rows, as zs_layernorm's rows): row m of dy is the
 * gradient of row rows[m] of x, and dx / res are addressed by rows[m] too; rows that repeat must
 * carry equal results (the caller zeroes dx first; rows not named stay untouched). */
int zs_layernorm_bwd(const float* x, int M, int C, int ldx, const int* rows, const float* dy,
                     int ldy, const float* g, float eps, const float* res, int ldr, float* dx,
                     int ldd, void* stream);

/* zs_gelu_tanh_bwd: du = gelu_new'(u) dh from the pre-activation u (HF GPT2MLP's activation,
 * which zs_gemm's ACT_GELU_TANH fuses); u / du dtype, dh f32. */
int zs_gelu_tanh_bwd(const void* u, const float* dh, long n, void* du, int dtype, void* stream);
/* zs_tanh_bwd: dpre = (1 - h^2) dh, the mapper's nn.Tanh (mapper.py:6-18) from its output h. */
int zs_tanh_bwd(const float* h, const float* dh, long n, float* dpre, void* stream);

/* zs_nll_grad_rows: the gradient of the mean cross-entropy (train_prompt.py:133) at the LM
 * head's input rows, from mix[m] = sum_v softmax(logit[m])_v wte[v] (zs_memory_project +
 * zs_memory_merge over the bank wte, scale 1, not normalised):
 *   dhf[m] = (mix[m] - wte[tgt[m]]) / sum_b cnt[b], zeros for tgt[m] outside [0, V);
 * cnt [B] are the device's caption lengths (zs_nll_finalize). */
int zs_nll_grad_rows(const float* mix, int ldm, const void* wte, int V, int K, const int* tgt,
                     const int* cnt, int B, int M, float* dhf, int ldd, int dtype, void* stream);
/* zs_nll_loss: loss[0] = -sum_b sum[b] / sum_b cnt[b] of zs_nll_finalize's per-caption sums,
 * the batch's mean token cross-entropy (train_prompt.py:133), on the device. */
int zs_nll_loss(const float* sum, const int* cnt, int B, float* loss, void* stream);
/* zs_soft_grad_rows: d_soft[b][j*D + d] = dx[(b*Smax + H_b + j)*D + d], j < n_soft: the
 * residual-stream gradient at the soft-prefix rows of zs_gpt2_score_embed's layout (the
 * backward of the concatenation, caption_model.py:303-306); H_b = hard_len[b] cut to [0, h_cap]. */
int zs_soft_grad_rows(const float* dx, const int* hard_len, int h_cap, int n_soft, int B, int Smax,
                      int D, float* d_soft, int ld, void* stream);

/* zs_colsum: out[n] = sum_b x[b][n] in row order (the bias gradients of the mapper's two
 * nn.Linear, mapper.py:6-18). */
int zs_colsum(const float* x, int B, int N, int ldx, float* out, void* stream);
/* zs_transpose_cast: y [C][Rp] (dtype) = x [R][C]^T (f32), Rp = R rounded up to 32, columns
 * R .. Rp-1 zero: the operand form zs_gemm takes for dX = dY W (a transposed weight) and for
 * dW = dY^T X (K = the padded batch). */
int zs_transpose_cast(const float* x, int R, int C, int ldx, void* y, int Rp, int dtype,
                      void* stream);

/* zs_adamw: one torch.optim.AdamW update (train_prompt.py:104) of n elements on the f32 master
 * p with moments m, v:  p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
 * p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps);  step >= 1.  operand (may be
 * NULL): the dtype copy the forward's GEMMs read, refreshed from the new p.  step_ctr (may be
 * NULL): step_ctr[0] = step. */
int zs_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
             float beta2, float eps, float weight_decay, int step, void* operand, int dtype,
             int* step_ctr, void* stream);

/* zs_noise_inject: noise_injection (utils.py:19-31): variance == 0 copies x to out; else
 * out = normalize(normalize(x) + sqrt(variance) n), n ~ N(0, 1) iid (F.normalize, eps 1e-12).
 * n of row r, columns 4c .. 4c+3: Philox4x32-10 with key = seed and counter (row_id[r] (NULL: r),
 * step_ctr[0] (NULL: 0), c, 0); words (0, 1) and (2, 3) each give two normals by Box-Muller,
 * u1 = ((w >> 8) + 1) 2^-24, u2 = (w' >> 8) 2^-24, (r cos, r sin)(2 pi u2), r = sqrt(-2 ln u1).
 * A row's noise depends on its id and the step, not on its slot in the launch.  out may be x. */
int zs_noise_inject(const float* x, int B, int D, int ldx, const int* row_id, const int* step_ctr,
                    long seed, float variance, float* out, int ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZSAAC_H */
