/*
 * tts_mi355x_ops.h — op-level entry points of the same library, used by the parity tests
 * to check each kernel family in isolation against the CPU oracle.  All pointers are
 * device pointers of the current HIP device; `stream` is a hipStream_t (NULL = default).
 * These are not part of the drop-in surface (tts_mi355x.h) and may change between rounds.
 */
#ifndef TTS_MI355X_OPS_H
#define TTS_MI355X_OPS_H

#include <stdint.h>
#include "tts_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Deterministic synthetic weights: value_i = (2*u_i - 1) * scale, u_i = top 24 bits of
 * splitmix64(seed + (i+1)*golden) / 2^24.  dtype TTS_DT_F32 or TTS_DT_BF16 (RNE).  Bit-identical
 * to tts_amd.synth.synth_values (numpy). */
tts_status tts_synth_fill(void* dst, int32_t dtype, int64_t n, uint64_t seed, float scale,
                          void* stream);

/* W [N][K] bf16 row-major -> 1 KiB MFMA fragment tiles in the matrix's stream-plan order
 * (layout in lm_kernels.h / lm_gemm.hip).  epi = the epilogue the matrix will be used with:
 * 2 (SwiGLU) takes W = [gate; up] ([N/2][K] each) and interleaves their n-tiles. */
tts_status tts_op_retile(const void* w, void* w_tiled, int32_t N, int32_t K, int32_t epi, void* stream);

/* y[M][ldo] (bf16) = epilogue( A[M][K] . W^T ), A optionally RMSNorm'ed with normw.
 * epi: 0 store, 1 residual (resid += y, in place), 2 SwiGLU (W = interleaved gate/up tiles,
 * N = 2*intermediate, output [M][N/2]).  M <= 64. */
tts_status tts_op_wgemm(const void* x, int32_t M, int32_t K, int32_t ldx, const void* w_tiled,
                        int32_t N, const void* normw, float eps, void* out, int32_t ldo,
                        void* resid, int32_t epi, void* stream);

/* Prefill GEMM (many rows, one launch): same tiled weights and epilogues as tts_op_wgemm
 * (0 store, 1 residual, 2 SwiGLU), no fused RMSNorm, any M >= 1; N % 64 == 0, K % 128 == 0.
 * Every output sums its K in the canonical 1024-element chunks, in order, so a row's bits do
 * not depend on M or on the launch form (all of K per workgroup / one chunk per workgroup).
 * Replaces the per-token projections of transformers LlamaForCausalLM.forward over the
 * prompt (modeling_llama.py:163-176, 217-281) when the whole prompt batch is prefilled. */
tts_status tts_op_pgemm(const void* x, int32_t M, int32_t K, const void* w_tiled, int32_t N, void* out,
                        int32_t ldo, void* resid, int32_t epi, void* stream);

/* The lm_head with the pick's epilogue, alone, on caller-owned device buffers: for every row m of
 * x [M][K] (bf16; RMSNorm'ed with normw / eps first when normw is not NULL) and column n of the
 * tiled head (tts_op_retile, epi 0; N % 64 == 0, K % 128 == 0, M in 1..256)
 *   v = bf16(x[m] . W[n]) as fp32;  bit n of seen[m] set: v = v < 0 ? v * penalty : v / penalty;
 *   counts not NULL: v -= freq_penalty * counts[m][n];  n == eos_mask[m]: v = -inf
 * (seen: [M][seen_stride] words, seen_stride >= N / 32; counts: uint16 [M][seen_stride * 32];
 * eos_mask: int32 [M], -1 = none).  row_penalty / row_freq (both or neither; float [M], counts
 * required): the per-row form, row m's penalties from the arrays instead of the scalars.
 * Outputs: part_val / part_idx [M][1024], of which the first *nparts (host int) entries of a row
 * are (maximum, lowest id holding it) of disjoint column sets that together cover every column —
 * what finalize and the samplers reduce; logits_out (optional) fp32 [M][N], every v.
 * form 0: the tile head of the 65..256-row decode step (lm_pgemm.hip head_tile_kernel): one
 * launch, K summed in the canonical 1024-element chunks — bf16(sum) equals tts_op_pgemm's epi 0
 * output bit for bit, at every M.  form 1: the decode head as the engine runs it up to 64 rows,
 * in launches of 32 rows (the decode stream's K order; K % 256 == 0). */
tts_status tts_op_head_pick(const void* x, int32_t M, int32_t K, const void* normw, float eps, const void* w_tiled,
                            int32_t N, const uint32_t* seen, int32_t seen_stride, float penalty,
                            const uint16_t* counts, float freq_penalty, const int32_t* eos_mask,
                            const float* row_penalty, const float* row_freq, float* part_val, int32_t* part_idx,
                            int32_t* nparts, float* logits_out, int32_t form, void* stream);

/* Sampling head (GenerationMixin._sample with TemperatureLogitsWarper, TopKLogitsWarper,
 * TopPLogitsWarper; transformers logits_process.py:238,473,542): rows of processed fp32
 * logits [B][V] -> one drawn token per row (tokens, device int32 [B]) and, when `probs` is
 * not NULL, the final distribution written into probs [B][V] at the kept ids (the caller
 * zero-fills it).  part_max (optional, [B][nparts]) = maxima of disjoint column blocks of
 * each row, used as the top-k lower bound the engine gets from its lm_head workgroups.
 * The draw is u = splitmix64(seed, row, step) in [0,1) walked over the kept ids in
 * descending-probability order (distribution-exact; not torch's RNG stream). */
tts_status tts_op_sample(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k,
                         float top_p, uint64_t seed, int32_t step, const float* part_max, int32_t nparts,
                         float* probs, int32_t* tokens, void* stream);

/* The same draw from per-row candidate lists instead of dense rows (the screened sampled step's
 * sampler, alone): row b is counts[b] (<= cap) entries scores[b][i] (processed fp32 logits) of
 * the ids ids[b][i] (distinct, in [0, V)), rows `cap` entries apart; every id not listed counts
 * as -inf.  A list that holds every entry of the row's top-k set gives the token and the probs
 * (written into probs [B][V] at the kept ids; the caller zero-fills it) of tts_op_sample on the
 * dense row, bit for bit.  Lists longer than the kernel's 2048 LDS candidates take the exact
 * radix select over the list.  An empty list (counts[b] == 0) has nothing to draw from: token 0,
 * no probs.  counts is only read. */
tts_status tts_op_sample_list(const float* scores, const int32_t* ids, const int32_t* counts, int32_t B,
                              int32_t cap, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                              int32_t step, float* probs, int32_t* tokens, void* stream);

/* The per-row samplers of the per-request slot batch, alone: row b samples with temperature[b],
 * top_k[b] (1..1024), top_p[b] and the key row_seed[b] (the draw of tts_op_sample with that seed on
 * the row alone: u = splitmix64(row_seed[b], 0, step)) when sample[b] != 0; sample[b] == 0 is a
 * greedy row: the argmax by float comparison, lowest id on ties (+0.0 and -0.0 tie), untouched by
 * the temperature, and no probs.  The five settings arrays are device arrays of B entries (the
 * kernel reads them; nothing checks their values).  ids NULL: dense rows scores [B][V] (cap
 * unused); part_max / part_idx [B][nparts] are optional, as in tts_op_sample (a greedy row then
 * reduces the partials instead of the row).  ids set: candidate lists as tts_op_sample_list
 * (counts required, only read; part_* unused).  probs optional. */
tts_status tts_op_sample_rows(const float* scores, const int32_t* ids, const int32_t* counts, int32_t B, int32_t cap,
                              int32_t V, const float* temperature, const int32_t* top_k, const float* top_p,
                              const int32_t* sample, const uint64_t* row_seed, int32_t step, const float* part_max,
                              const int32_t* part_idx, int32_t nparts, float* probs, int32_t* tokens, void* stream);

/* Diagnostics, no GPU needed: the kernels one decode step over `rows` rows (1..256) of a model of
 * config `cfg` would launch on a GPU of `num_cu` CUs — the engine's own step code run with
 * its launchers in a dry-run mode (nothing allocated or launched).  Writes the unique launches
 * in first-seen order, one per line (the weight-streaming GEMMs as
 * "wgemm_kernel<template arguments>"; from 65 rows the tile GEMMs "pgemm_kernel<MW, NW, EPI>" and
 * the tile lm_head "head_tile_kernel<MW, per-row>"), NUL-terminated, into out[cap].  The build's spill gate
 * (tests/test_kernel_resources.py) reads its hot instantiations from here. */
tts_status tts_debug_step_plan(const tts_lm_config* cfg, int32_t rows, int32_t num_cu, char* out, int32_t cap);
/* Diagnostics, no GPU needed: the decode GEMM's plan for an M x N x K launch with epilogue epi
 * (0 store, 1 residual, 2 SwiGLU, 3 / 4 lm_head) on a GPU of num_cu CUs, as out[8] = {layout
 * units, units per layout round (ur), launch grid, K chunks (kc), csplit, K-sliced, A rows in
 * LDS, launch shape index}: units > ur with units % ur != 0 is a partial last round. */
tts_status tts_debug_wgemm_plan(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t num_cu, int32_t* out);
/* Diagnostics, no GPU needed: what the warm workgroups of the one-row fused QKV + attention +
 * o_proj launch read of the tiled 2 FF x hidden gate/up matrix (N x K, the one-row SwiGLU plan
 * on num_cu CUs): `stages` stages of every gate/up workgroup's stream, dealt over `wgs` warm
 * workgroups (0, or at least 8), warm workgroup b taking the gate/up blocks g with g mod 8 ==
 * (b + shift) mod 8.  info[8] = {stages after clamping, warm workgroups, gate/up workgroups,
 * bytes of one workgroup's stage block, of the last workgroup's, bytes between stages, shift mod
 * 8, stages per item}; out[cap][5] = {warm workgroup, byte offset, bytes, gate/up block, stage}
 * per range, *n of them. */
tts_status tts_debug_warm_plan(int32_t N, int32_t K, int32_t num_cu, int32_t stages, int32_t wgs, int32_t shift,
                               int32_t* info, int64_t* out, int32_t cap, int32_t* n);
/* ... of a sampled step (do_sample at temperature 0.8, top_p 1.0 and the given top_k in [1, 1024]):
 * the screened sampling head where it applies (head_screen_kernel<..., true> + sample_list_kernel),
 * else the full lm_head with its logits store (65..256 rows: the tile lm_head) + sample_kernel. */
tts_status tts_debug_step_plan_sampled(const tts_lm_config* cfg, int32_t rows, int32_t num_cu, int32_t top_k,
                                       char* out, int32_t cap);

/* ... of the per-request batch's step (tts_slots_open_per_request) whose largest admitted top_k is
 * max_top_k: the screen's per-row top-k variant (head_screen_kernel<MT, KT8, rows per wave + 8, false, true>) +
 * sample_list_rows_kernel where the rows and max_top_k fit the screen, else the full lm_head with
 * the per-row epilogue (wgemm_kernel<..., 4, ...>; 65..256 rows: head_tile_kernel<MW, true>) +
 * sample_rows_kernel. */
tts_status tts_debug_step_plan_rows(const tts_lm_config* cfg, int32_t rows, int32_t num_cu, int32_t max_top_k,
                                    char* out, int32_t cap);

/* LlamaRMSNorm over rows of x (bf16). */
tts_status tts_op_rmsnorm(const void* x, const void* w, float eps, void* y, int32_t M, int32_t K,
                          void* stream);

/* SpeechLM attention alone (lm_attn.hip; LlamaAttention.forward after the projections:
 * apply_rotary_pos_emb in bf16, the KV cache append, GQA 4:1 causal SDPA).  Common arguments:
 * qkv = bf16 rows [rows][ld_qkv] laid out q (H*D) | k (KVH*D) | v (KVH*D), ld_qkv >= (H + 2 KVH) D
 * and a multiple of 8; kcache = K rows [n_slots][KVH][max_seq][D]; vtcache = V^T
 * [n_slots][KVH] blocks of D x max_seq in tiles of 16 dimensions x 32 positions (element (d, p) at
 * (((d / 16) * (max_seq / 32) + p / 32) * 16 + d % 16) * 32 + p % 32); rope_cos / rope_sin = bf16
 * tables [max_seq][D]; out = bf16 [rows][H*D].  Rejected with an error and no launch: D not 64 or
 * 128, H != 4 KVH, max_seq not a multiple of 64, a slot outside [0, n_slots) or used by two rows /
 * sequences, a position >= max_seq.
 *
 * Prefill: n_seq sequences (host arrays seq_slot, seq_pos0, seq_len); sequence b's seq_len[b]
 * consecutive qkv rows are positions seq_pos0[b] .. + seq_len[b] - 1 of slot seq_slot[b]
 * (seq_pos0 > 0: positions below it are already in the cache).  Runs the engine's RoPE + append
 * launch (roped q -> q_rot [rows][H*D], roped k and v into the caches), then its causal
 * attention launch over 16-row query blocks built as the engine builds them.  KVH <= 8.
 * Returns after the stream has drained. */
tts_status tts_op_attn_prefill(const void* qkv, int32_t ld_qkv, const int32_t* seq_slot, const int32_t* seq_pos0,
                               const int32_t* seq_len, int32_t n_seq, int32_t n_slots, void* kcache,
                               void* vtcache, int32_t max_seq, const void* rope_cos, const void* rope_sin,
                               int32_t H, int32_t KVH, int32_t D, float scale, void* q_rot, void* out,
                               void* stream);

/* Decode step: row r (device int32 arrays row_slot, row_pos) is the new position row_pos[r] of
 * slot row_slot[r]; it attends positions 0 .. row_pos[r] (the earlier ones from the caches, its
 * own from the row) and is appended to the caches.  The rows come from qkv, or (qkv NULL) from
 * qkv_part = fp32 partials [qkv_nsl][rows][ld_qkv] of a K-sliced projection, summed in slice
 * order and rounded once to bf16. */
tts_status tts_op_attn_decode(const void* qkv, const float* qkv_part, int32_t qkv_nsl, int32_t ld_qkv,
                              int32_t rows, const int32_t* row_slot, const int32_t* row_pos, int32_t n_slots,
                              void* kcache, void* vtcache, int32_t max_seq, const void* rope_cos,
                              const void* rope_sin, int32_t H, int32_t KVH, int32_t D, float scale, void* out,
                              void* stream);

/* fp32 GEMM on the codec path: C[M][N] = act(A[M][K] . B[N][K]^T + bias) (+ resid).
 * lda may be < K to express a sliding-window (im2col-free) conv operand.  act: 0 none,
 * 1 swish, 2 silu (same function), see codec_gemm.hip. */
tts_status tts_op_gemm_f32(const float* A, int32_t M, int32_t K, int32_t lda, const float* B,
                           int32_t N, const float* bias, float* C, int32_t ldc,
                           const float* resid, int32_t act, void* stream);

/* planes[0..3n) = the (h, m, l) bf16 split of x[0..n) the codec GEMMs apply to their operands
 * (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even; h + m + l == x):
 * split_planes_kernel alone, as the engine runs it over the weights at load. */
tts_status tts_op_split_planes(const float* x, uint16_t* planes, int64_t n, void* stream);

/* One codec GEMM kernel form alone: C[M][ldc] = act(A . B^T + bias) (+ resid), every operand the
 * engine's GemmF32Args carries.  A [M rows, lda apart][K] fp32 and / or Ap, its bf16 planes with
 * A's addressing (element (m, k) of plane p at Ap + p * ap_plane + m * lda + k); B [N][K] fp32
 * and / or Bp = planes [3][N][K] (tts_op_split_planes); bias [N], resid [M][ldc] optional; act 0
 * none, 1 swish.  Output: C fp32 and / or Cp, the planes of the stored value (element (m, n) of
 * plane p at Cp + p * cp_plane + m * ldc + n).  lda may be < K (the sliding-window conv operand).
 *
 * form -1: the engine's own choice, through its two wrappers: A NULL (Ap, Bp) -> launch_gemm_x3p
 * (tile by size and TTS_CODEC_X3P_*), else (A, B, optional Bp / Ap) -> launch_gemm_f32.
 * Any other value names one instantiation:
 *   gemm_x3p_kernel (Ap and Bp): tile | schedule << 3 | 0x20 (PP) | 0x40 (four stages), tile 0..5 =
 *     256x128, 128x128, 128x64, 64x64, 32x32, 128x128 on 8 waves with three stages; schedule 0 =
 *     two-stage DMA (ILV off), 1 = one stage ahead between the MFMAs (ILV on), 2 = the tile's own.
 *     PP exists on tile 0 with ILV, four stages on tile 4, three and four stages with ILV only.
 *   gemm_bx3_kernel: 0x100 + i, i = 0 256x128 Ap Bp, 1 128x128 Ap Bp, 2 256x128 A Bp,
 *     3 128x256 A Bp, 4 128x128 A Bp, 5 64x64 A Bp, 6 128x128 A B, 7 64x64 A B.
 *   gemm_f32_kernel (fp32 MFMA; A, B): 0x200 + i, i = 0 64x64 K step 64, 1 64x64 K step 16,
 *     2 128x128 K step 32, 3 128x128 K step 16.
 * Rejected with an error and no launch: an operand the form reads missing, K % 32 != 0 for a
 * bf16-split form (K no multiple of the K step for an fp32 form), PP / four stages / ILV off on a
 * tile that has no such kernel, lda % 8 != 0 or a base or plane stride off 16 bytes for planes
 * (lda % 4, 16 bytes for fp32 operands), an unknown form. */
tts_status tts_op_gemm_planes(const float* A, const uint16_t* Ap, int64_t ap_plane, int32_t M, int32_t K, int32_t lda,
                              const float* B, const uint16_t* Bp, int32_t N, const float* bias, float* C,
                              uint16_t* Cp, int64_t cp_plane, int32_t ldc, const float* resid, int32_t act,
                              int32_t form, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTS_MI355X_OPS_H */
