// capi.cpp — the extern "C" boundary (include/tts_mi355x.h, include/tts_mi355x_ops.h).
// Every entry point catches everything: errors become a status code plus a thread-local
// message, never an exception across the ABI.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>

#include "../../include/tts_mi355x.h"
#include "../../include/tts_mi355x_ops.h"
#include "codec_kernels.h"
#include "engine.h"

namespace tts {

static thread_local std::string g_last_error;

template <class F>
static tts_status guarded(F&& f) {
  try {
    f();
    return TTS_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return TTS_E_INVALID;
  } catch (...) {
    g_last_error = "unknown error";
    return TTS_E_INVALID;
  }
}

hipStream_t pick_stream(Engine* e, void* s) { return s ? (hipStream_t)s : e->stream; }

Engine::~Engine() {
  if (w.graph) (void)hipGraphExecDestroy(w.graph);
  if (w.h_active) (void)hipHostFree(w.h_active);
  if (codec) codec_destroy(codec);
  if (encoder) encoder_destroy(encoder);
  for (auto& v : ev)
    if (v) (void)hipEventDestroy(v);
  if (stream) (void)hipStreamDestroy(stream);
}

}  // namespace tts

using namespace tts;

extern "C" {

int32_t tts_abi_version(void) { return TTS_ABI_VERSION; }

const char* tts_last_error(void) { return g_last_error.c_str(); }

tts_status tts_engine_create(int32_t device, tts_engine** out) {
  return guarded([&] {
    TTS_REQUIRE(out != nullptr, "null output pointer");
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    TTS_REQUIRE(device >= 0 && device < n, "device index out of range");
    HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<Engine> e(new Engine());  // freed if a HIP call below throws
    e->device = device;
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    e->num_cu = prop.multiProcessorCount;
    HIP_CHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    for (auto& v : e->ev) HIP_CHECK(hipEventCreate(&v));
    *out = reinterpret_cast<tts_engine*>(e.release());
  });
}

void tts_engine_destroy(tts_engine* e) {
  if (!e) return;
  Engine* E = reinterpret_cast<Engine*>(e);
  (void)hipSetDevice(E->device);
  (void)hipDeviceSynchronize();
  delete E;
}

tts_status tts_lm_load(tts_engine* e, const tts_lm_config* cfg, const tts_tensor_desc* t,
                       int32_t n) {
  return guarded([&] {
    TTS_REQUIRE(e && t && n > 0, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_load(E, cfg, t, n);
  });
}

tts_status tts_generate(tts_engine* e, const tts_gen_params* p, const int32_t* prompt_ids,
                        const int32_t* prompt_lens, int32_t batch, int32_t* out_ids,
                        int32_t out_stride, int32_t* out_lens, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && p && prompt_ids && prompt_lens && out_ids && out_lens, "null argument");
    TTS_REQUIRE(batch >= 1, "batch must be >= 1");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_generate(E, p, prompt_ids, prompt_lens, batch, out_ids, out_stride, out_lens,
                pick_stream(E, stream));
  });
}

tts_status tts_generate_begin(tts_engine* e, const tts_gen_params* p, const int32_t* prompt_ids,
                              const int32_t* prompt_lens, int32_t batch, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && p && prompt_ids && prompt_lens, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_gen_begin(E, p, prompt_ids, prompt_lens, batch, pick_stream(E, stream));
  });
}

tts_status tts_generate_continue(tts_engine* e, int32_t n_steps, int32_t* all_done) {
  return guarded([&] {
    TTS_REQUIRE(e && all_done && n_steps >= 0, "bad argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    *all_done = lm_gen_continue(E, n_steps);
  });
}

tts_status tts_generate_read(tts_engine* e, int32_t* out_ids, int32_t out_stride, int32_t* out_lens) {
  return guarded([&] {
    TTS_REQUIRE(e && out_ids && out_lens, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_gen_read(E, out_ids, out_stride, out_lens);
  });
}

tts_status tts_slots_open(tts_engine* e, const tts_gen_params* p, int32_t n_slots, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && p, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_open(E, p, n_slots, pick_stream(E, stream));
  });
}

tts_status tts_slots_open_per_request(tts_engine* e, const tts_gen_params* defaults, int32_t n_slots, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && defaults, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_open(E, defaults, n_slots, pick_stream(E, stream), true);
  });
}

tts_status tts_slots_add_params(tts_engine* e, int32_t slot, const int32_t* prompt_ids, int32_t prompt_len,
                                int32_t max_new_tokens, const tts_gen_params* p, const uint64_t* seed) {
  return guarded([&] {
    TTS_REQUIRE(e && prompt_ids, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_add(E, slot, prompt_ids, prompt_len, max_new_tokens, seed, p);
  });
}

tts_status tts_slots_add(tts_engine* e, int32_t slot, const int32_t* prompt_ids, int32_t prompt_len,
                         int32_t max_new_tokens) {
  return guarded([&] {
    TTS_REQUIRE(e && prompt_ids, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_add(E, slot, prompt_ids, prompt_len, max_new_tokens, nullptr);
  });
}

tts_status tts_slots_add_seeded(tts_engine* e, int32_t slot, const int32_t* prompt_ids, int32_t prompt_len,
                         int32_t max_new_tokens, uint64_t seed) {
  return guarded([&] {
    TTS_REQUIRE(e && prompt_ids, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_add(E, slot, prompt_ids, prompt_len, max_new_tokens, &seed);
  });
}

tts_status tts_slots_step(tts_engine* e, int32_t n_steps, int32_t* n_active) {
  return guarded([&] {
    TTS_REQUIRE(e && n_active && n_steps >= 0, "bad argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    *n_active = lm_slots_step(E, n_steps);
  });
}

tts_status tts_slots_read(tts_engine* e, int32_t slot, int32_t* out_ids, int32_t capacity, int32_t* n_out,
                          int32_t* finished) {
  return guarded([&] {
    TTS_REQUIRE(e && out_ids && n_out && finished, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_read(E, slot, out_ids, capacity, n_out, finished);
  });
}

tts_status tts_slots_release(tts_engine* e, int32_t slot) {
  return guarded([&] {
    TTS_REQUIRE(e, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_slots_release(E, slot);
  });
}

tts_status tts_lm_score(tts_engine* e, const int32_t* ids, const int32_t* lens, int32_t batch,
                        int32_t n_last, float* logits, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && ids && lens && logits && n_last >= 1, "bad argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_score(E, ids, lens, batch, n_last, logits, pick_stream(E, stream));
  });
}

tts_status tts_lm_score_decode(tts_engine* e, const int32_t* ids, const int32_t* lens, int32_t batch,
                               int32_t n_last, const int32_t* gather_idx, int32_t k, float* logits,
                               void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && ids && lens && logits && n_last >= 1, "bad argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_score_decode(E, ids, lens, batch, n_last, gather_idx, k, logits, pick_stream(E, stream));
  });
}

tts_status tts_lm_id_to_code(tts_engine* e, const int32_t* ids, int32_t n, int32_t* codes) {
  return guarded([&] {
    TTS_REQUIRE(e && ids && codes && n >= 0, "bad argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    TTS_REQUIRE(!E->lm.id_to_code.empty(), "no vocab.id_to_code LUT was loaded");
    const int V = (int)E->lm.id_to_code.size();
    for (int i = 0; i < n; ++i) codes[i] = (ids[i] >= 0 && ids[i] < V) ? E->lm.id_to_code[ids[i]] : -1;
  });
}

tts_status tts_lm_last_timing(tts_engine* e, float* prefill_ms, float* decode_ms,
                              int32_t* decode_steps) {
  return guarded([&] {
    TTS_REQUIRE(e, "null engine");
    Engine* E = reinterpret_cast<Engine*>(e);
    if (prefill_ms) *prefill_ms = E->t_prefill_ms;
    if (decode_ms) *decode_ms = E->t_decode_ms;
    if (decode_steps) *decode_steps = E->decode_steps;
  });
}

tts_status tts_lm_bench_kernel(tts_engine* e, int32_t which, int32_t rows, int32_t ctx,
                               int32_t iters, float* avg_ms, double* bytes) {
  return guarded([&] {
    TTS_REQUIRE(e && avg_ms && bytes, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    lm_bench_kernel(E, which, rows, ctx, iters, avg_ms, bytes);
  });
}

tts_status tts_debug_step_plan(const tts_lm_config* cfg, int32_t rows, int32_t num_cu, char* out, int32_t cap) {
  return guarded([&] {
    TTS_REQUIRE(cfg && out && cap > 0, "null argument");
    const std::string p = lm_step_plan(*cfg, rows, num_cu);
    TTS_REQUIRE((int64_t)p.size() < cap, "output buffer too small");
    memcpy(out, p.c_str(), p.size() + 1);
  });
}

tts_status tts_debug_wgemm_plan(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t num_cu, int32_t* out) {
  return guarded([&] {
    TTS_REQUIRE(out && num_cu > 0, "null argument");
    TTS_REQUIRE(epi >= EPI_STORE && epi <= EPI_LOGITS_ROWS && wgemm_supported(M, N, K, epi), "unsupported GEMM shape");
    const WgemmPlan p = plan_wgemm(M, N, K, epi, num_cu);
    out[0] = (N / 16) / p.sp.ng;  // layout units
    out[1] = p.sp.ur();           // units per round of the layout
    out[2] = p.grid;
    out[3] = p.sp.kc;
    out[4] = p.csplit;
    out[5] = p.sliced ? 1 : 0;
    out[6] = p.a_lds ? 1 : 0;
    out[7] = p.cfg;
  });
}

tts_status tts_debug_warm_plan(int32_t N, int32_t K, int32_t num_cu, int32_t stages, int32_t wgs, int32_t shift,
                               int32_t* info, int64_t* out, int32_t cap, int32_t* n) {
  return guarded([&] {
    TTS_REQUIRE(info && out && n && num_cu > 0 && cap >= 0, "null argument");
    TTS_REQUIRE(wgemm_supported(1, N, K, EPI_SWIGLU), "unsupported GEMM shape");
    const WgemmPlan p = plan_wgemm(1, N, K, EPI_SWIGLU, num_cu);
    const WarmArgs a = wgemm_warm_plan(p, nullptr, N, K, stages, wgs, shift);
    const int32_t v[8] = {a.stages, a.wgs, a.nblk, (int32_t)a.blk_bytes, (int32_t)a.last_bytes, (int32_t)a.stage_bytes,
                          a.shift, (K / 32) / (p.sp.ksplit * p.sp.ku)};
    memcpy(info, v, sizeof v);
    int rows = 0;
    for (int b = 0; b < a.wgs; ++b)
      warm_walk(a, b, [&](uint32_t off, uint32_t len, int g, int st) {
        TTS_REQUIRE(rows < cap, "output buffer too small");
        int64_t* r = out + (size_t)rows++ * 5;
        r[0] = b; r[1] = off; r[2] = len; r[3] = g; r[4] = st;
      });
    *n = rows;
  });
}

tts_status tts_debug_step_plan_sampled(const tts_lm_config* cfg, int32_t rows, int32_t num_cu, int32_t top_k,
                                       char* out, int32_t cap) {
  return guarded([&] {
    TTS_REQUIRE(cfg && out && cap > 0, "null argument");
    TTS_REQUIRE(top_k >= 1 && top_k <= SAMPLE_MAX_TOP_K, "top_k in [1, 1024]");
    const std::string p = lm_step_plan(*cfg, rows, num_cu, top_k);
    TTS_REQUIRE((int64_t)p.size() < cap, "output buffer too small");
    memcpy(out, p.c_str(), p.size() + 1);
  });
}

tts_status tts_debug_step_plan_rows(const tts_lm_config* cfg, int32_t rows, int32_t num_cu, int32_t max_top_k,
                                    char* out, int32_t cap) {
  return guarded([&] {
    TTS_REQUIRE(cfg && out && cap > 0, "null argument");
    TTS_REQUIRE(max_top_k >= 1 && max_top_k <= SAMPLE_MAX_TOP_K, "max_top_k in [1, 1024]");
    const std::string p = lm_step_plan(*cfg, rows, num_cu, max_top_k, true);
    TTS_REQUIRE((int64_t)p.size() < cap, "output buffer too small");
    memcpy(out, p.c_str(), p.size() + 1);
  });
}

tts_status tts_codec_load(tts_engine* e, const tts_codec_config* cfg, const tts_tensor_desc* t,
                          int32_t n) {
  return guarded([&] {
    TTS_REQUIRE(e && cfg && t && n > 0, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    codec_load(E, cfg, t, n);
  });
}

tts_status tts_codec_decode(tts_engine* e, const int32_t* codes, const int32_t* lens,
                            int32_t batch, float* wav, int32_t wav_is_device, int64_t* wav_lens,
                            void* stream) {
  return guarded([&] {
    TTS_REQUIRE(e && codes && lens && wav && wav_lens && batch >= 1, "bad argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    codec_decode(E, codes, lens, batch, wav, wav_is_device, wav_lens, pick_stream(E, stream));
  });
}

tts_status tts_encoder_load(tts_engine* e, const tts_tensor_desc* t, int32_t n) {
  return guarded([&] {
    TTS_REQUIRE(e && t && n > 0, "null argument");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    encoder_load(E, t, n);
  });
}

tts_status tts_encoder_encode(tts_engine* e, const float* wav, int64_t n_samples, const float* w2v_features,
                              int32_t n_frames, int32_t* codes, int32_t codes_cap, int32_t* n_codes,
                              float* pre_round) {
  return guarded([&] {
    TTS_REQUIRE(e && wav && w2v_features && codes && n_codes, "null argument");
    TTS_REQUIRE(n_samples >= 1 && n_samples < (1ll << 31) - 640, "bad waveform length");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    *n_codes = encoder_encode(E, wav, (int)n_samples, w2v_features, n_frames, codes, codes_cap, pre_round);
  });
}

tts_status tts_encoder_encode_features(tts_engine* e, const float* wav, int64_t n_samples, const float* features,
                                       int32_t n_frames, int32_t* codes, int32_t codes_cap, int32_t* n_codes,
                                       float* pre_round) {
  return guarded([&] {
    TTS_REQUIRE(e && wav && features && codes && n_codes, "null argument");
    TTS_REQUIRE(n_samples >= 1 && n_samples < (1ll << 31) - 640, "bad waveform length");
    Engine* E = reinterpret_cast<Engine*>(e);
    HIP_CHECK(hipSetDevice(E->device));
    *n_codes = encoder_encode(E, wav, (int)n_samples, nullptr, n_frames, codes, codes_cap, pre_round, features);
  });
}

tts_status tts_codec_samples_per_code(tts_engine* e, int32_t* out) {
  return guarded([&] {
    TTS_REQUIRE(e && out, "null argument");
    *out = codec_samples_per_code(reinterpret_cast<Engine*>(e));
  });
}

// ------------------------------------------------------------------------ op level ----

tts_status tts_synth_fill(void* dst, int32_t dtype, int64_t n, uint64_t seed, float scale,
                          void* stream) {
  return guarded([&] {
    TTS_REQUIRE(dst && n >= 0 && (dtype == TTS_DT_F32 || dtype == TTS_DT_BF16), "bad argument");
    launch_synth_fill(dst, dtype == TTS_DT_F32 ? 0 : 1, n, seed, scale, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

static int device_cu_count() {  // (single-device process: cached, no per-call query)
  static int num_cu = 0;
  if (!num_cu) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
  }
  return num_cu;
}

tts_status tts_op_retile(const void* w, void* w_tiled, int32_t N, int32_t K, int32_t epi, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(w && w_tiled && N % (epi == EPI_SWIGLU ? 32 : 16) == 0 && K % 256 == 0, "bad argument");
    const int ncu = device_cu_count();
    if (epi == EPI_SWIGLU) {  // rows [0, N/2) = gate, [N/2, N) = up: n-tiles interleaved
      const bf16_t* wg = (const bf16_t*)w;
      launch_retile(wg, (bf16_t*)w_tiled, N / 2, K, N, 2, ncu, (hipStream_t)stream, 2, 0);
      launch_retile(wg + (size_t)(N / 2) * K, (bf16_t*)w_tiled, N / 2, K, N, 2, ncu, (hipStream_t)stream, 2, 1);
    } else {
      launch_retile((const bf16_t*)w, (bf16_t*)w_tiled, N, K, N, 1, ncu, (hipStream_t)stream, 1, 0);
    }
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_wgemm(const void* x, int32_t M, int32_t K, int32_t ldx, const void* w_tiled,
                        int32_t N, const void* normw, float eps, void* out, int32_t ldo,
                        void* resid, int32_t epi, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SWIGLU, "bad epilogue");
    TTS_REQUIRE(wgemm_supported(M, N, K, epi), "unsupported GEMM shape");
    TTS_REQUIRE(ldx == K, "ldx must equal K");
    WgemmPlan p = plan_wgemm(M, N, K, epi, device_cu_count());
    hipStream_t st = (hipStream_t)stream;
    WgemmArgs a;
    a.x = (const bf16_t*)x; a.M = M; a.K = K; a.ldx = ldx;
    a.w = (const bf16_t*)w_tiled; a.N = N;
    a.normw = (const bf16_t*)normw; a.eps = eps;
    a.out = (bf16_t*)out; a.ldo = ldo; a.resid = (bf16_t*)resid;
    // RMSNorm in the GEMM's prologue where the rows fit it (LDS rows, K <= 4096, the LDS-DMA
    // pieces of 512 columns); otherwise a standalone pass first — the same canonical sum order
    // (chunk_sumsq), so the same bits either way, as the engine does (lm_step.cpp Ctx::gemm)
    bf16_t* xn = nullptr;
    if (normw && !(p.a_lds && !p.sliced && K <= 4096 && K % 512 == 0)) {
      HIP_CHECK(hipMallocAsync((void**)&xn, (size_t)M * K * 2, st));
      launch_rmsnorm(a.x, ldx, a.normw, eps, xn, K, M, K, st);
      a.x = xn;
      a.normw = nullptr;
    }
    float* part = nullptr;
    if (p.sliced) {
      HIP_CHECK(hipMallocAsync((void**)&part, wgemm_part_elems(p, M, ldo) * 4, st));
      a.part_out = part;
    }
    launch_wgemm(a, p, epi, a.normw != nullptr, st);
    HIP_CHECK(hipGetLastError());
    if (part) HIP_CHECK(hipFreeAsync(part, st));
    if (xn) HIP_CHECK(hipFreeAsync(xn, st));
  });
}

tts_status tts_op_pgemm(const void* x, int32_t M, int32_t K, const void* w_tiled, int32_t N, void* out,
                        int32_t ldo, void* resid, int32_t epi, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(pgemm_supported(M, N, K, epi), "unsupported prefill GEMM shape / epilogue");
    TTS_REQUIRE(epi == EPI_RESID ? resid != nullptr : out != nullptr, "missing output");
    PgemmArgs a;
    a.x = (const bf16_t*)x; a.M = M; a.K = K; a.ldx = K;
    a.w = (const bf16_t*)w_tiled; a.N = N;
    a.out = (bf16_t*)out; a.ldo = ldo; a.resid = (bf16_t*)resid;
    // the engine's scratch for the one-chunk-per-workgroup form (prompts of <= 256 rows,
    // lm_load.cpp kPgemmSplitRows): a stream-ordered allocation of this call's size
    hipStream_t s = (hipStream_t)stream;
    if (M <= 256) {
      a.part_bytes = pgemm_part_bytes(M, N, K);
      HIP_CHECK(hipMallocAsync((void**)&a.part, a.part_bytes, s));
    }
    launch_pgemm(a, epi, device_cu_count(), s);
    HIP_CHECK(hipGetLastError());
    if (a.part) HIP_CHECK(hipFreeAsync(a.part, s));
  });
}

tts_status tts_op_head_pick(const void* x, int32_t M, int32_t K, const void* normw, float eps, const void* w_tiled,
                            int32_t N, const uint32_t* seen, int32_t seen_stride, float penalty,
                            const uint16_t* counts, float freq_penalty, const int32_t* eos_mask,
                            const float* row_penalty, const float* row_freq, float* part_val, int32_t* part_idx,
                            int32_t* nparts, float* logits_out, int32_t form, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(x && w_tiled && seen && eos_mask && part_val && part_idx && nparts, "null argument");
    TTS_REQUIRE(form == 0 || form == 1, "form: 0 the tile head, 1 the decode head in chunks of 32");
    TTS_REQUIRE(head_tile_supported(M, N, K), "M in [1, 256], N % 64 == 0, K % 128 == 0");
    TTS_REQUIRE(form == 0 || wgemm_supported(std::min(M, 32), N, K, EPI_LOGITS), "unsupported decode head shape");
    TTS_REQUIRE(seen_stride >= N / 32, "seen_stride below N / 32");
    TTS_REQUIRE((row_penalty != nullptr) == (row_freq != nullptr), "the rows form takes both per-row arrays");
    const bool rows = row_penalty != nullptr;
    TTS_REQUIRE(!rows || counts, "the rows form needs counts");
    hipStream_t s = (hipStream_t)stream;
    const int ncu = device_cu_count();
    const int epi = rows ? EPI_LOGITS_ROWS : EPI_LOGITS;
    // the rows normalised once by the standalone pass, as the engine does from 17 rows on
    bf16_t* xn = nullptr;
    const bf16_t* xin = (const bf16_t*)x;
    if (normw) {
      HIP_CHECK(hipMallocAsync((void**)&xn, (size_t)M * K * 2, s));
      launch_rmsnorm(xin, K, (const bf16_t*)normw, eps, xn, K, M, K, s);
      xin = xn;
    }
    RowParams* par = nullptr;
    if (rows) {  // the kernels read RowParams entries: a table from the two arrays
      std::vector<float> pen(M), frq(M);
      HIP_CHECK(hipMemcpyAsync(pen.data(), row_penalty, (size_t)M * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(frq.data(), row_freq, (size_t)M * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      std::vector<RowParams> tab(M);
      for (int m = 0; m < M; ++m) {
        TTS_REQUIRE(pen[m] > 0.f, "row penalties must be > 0");
        tab[m] = RowParams{pen[m], frq[m], 1.f, 1.f, 1, -1, 0, 0};
      }
      HIP_CHECK(hipMallocAsync((void**)&par, (size_t)M * sizeof(RowParams), s));
      HIP_CHECK(hipMemcpyAsync(par, tab.data(), (size_t)M * sizeof(RowParams), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));  // (tab is a local buffer)
    }
    if (form == 0) {
      HeadTileArgs h;
      h.g.x = xin; h.g.M = M; h.g.K = K; h.g.ldx = K;
      h.g.w = (const bf16_t*)w_tiled; h.g.N = N;
      h.seen = seen; h.seen_stride = seen_stride; h.penalty = penalty; h.eos_mask = eos_mask;
      h.part_val = part_val; h.part_idx = part_idx; h.part_stride = LOGITS_MAX_PARTS;
      h.logits_out = logits_out; h.ldl = N;
      h.counts = counts; h.freq_penalty = freq_penalty; h.row_par = par;
      launch_head_tile(h, rows, ncu, s);
      *nparts = head_tile_nparts(N);
    } else {
      for (int r0 = 0; r0 < M; r0 += 32) {
        const int m = std::min(32, M - r0);
        const WgemmPlan p = plan_wgemm(m, N, K, epi, ncu);
        TTS_REQUIRE(p.grid <= LOGITS_MAX_PARTS, "decode head grid above the partials' stride");
        WgemmArgs a;
        a.x = xin + (size_t)r0 * K; a.M = m; a.K = K; a.ldx = K;
        a.w = (const bf16_t*)w_tiled; a.N = N;
        a.seen = seen + (size_t)r0 * seen_stride; a.seen_stride = seen_stride; a.penalty = penalty;
        a.eos_mask = eos_mask + r0;
        a.part_val = part_val + (size_t)r0 * LOGITS_MAX_PARTS; a.part_idx = part_idx + (size_t)r0 * LOGITS_MAX_PARTS;
        a.part_stride = LOGITS_MAX_PARTS;
        if (logits_out) { a.logits_out = logits_out + (size_t)r0 * N; a.ldl = N; }
        if (counts) a.counts = counts + (size_t)r0 * seen_stride * 32;
        a.freq_penalty = freq_penalty;
        if (par) a.row_par = par + r0;
        launch_wgemm(a, p, epi, false, s);
        *nparts = p.grid;
      }
    }
    HIP_CHECK(hipGetLastError());
    if (par) HIP_CHECK(hipFreeAsync(par, s));
    if (xn) HIP_CHECK(hipFreeAsync(xn, s));
  });
}

tts_status tts_op_sample(const float* logits, int32_t B, int32_t V, float temperature, int32_t top_k,
                         float top_p, uint64_t seed, int32_t step, const float* part_max, int32_t nparts,
                         float* probs, int32_t* tokens, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(logits && tokens && B >= 1 && V >= 1, "bad arguments");
    TTS_REQUIRE(temperature > 0.f && top_k >= 1 && top_k <= SAMPLE_MAX_TOP_K && top_p > 0.f && top_p <= 1.f,
                "temperature > 0, top_k in [1, 1024], top_p in (0, 1]");
    SampleArgs a;
    a.logits = logits; a.ldl = V; a.V = V;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.step0 = step;
    a.part_val = part_max; a.nparts = part_max ? nparts : 0; a.part_stride = nparts;
    a.probs = probs; a.tokens = tokens;
    launch_sample(a, B, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_sample_list(const float* scores, const int32_t* ids, const int32_t* counts, int32_t B,
                              int32_t cap, int32_t V, float temperature, int32_t top_k, float top_p, uint64_t seed,
                              int32_t step, float* probs, int32_t* tokens, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(scores && ids && counts && tokens && B >= 1 && V >= 1 && cap >= 1, "bad arguments");
    TTS_REQUIRE(temperature > 0.f && top_k >= 1 && top_k <= SAMPLE_MAX_TOP_K && top_p > 0.f && top_p <= 1.f,
                "temperature > 0, top_k in [1, 1024], top_p in (0, 1]");
    SampleArgs a;
    a.logits = scores; a.list_idx = ids; a.list_cnt = const_cast<int32_t*>(counts);  // (list_clear 0: only read)
    a.ldl = cap; a.V = cap; a.vocab = V;
    a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.step0 = step;
    a.probs = probs; a.tokens = tokens;
    launch_sample_list(a, B, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_sample_rows(const float* scores, const int32_t* ids, const int32_t* counts, int32_t B, int32_t cap,
                              int32_t V, const float* temperature, const int32_t* top_k, const float* top_p,
                              const int32_t* sample, const uint64_t* row_seed, int32_t step, const float* part_max,
                              const int32_t* part_idx, int32_t nparts, float* probs, int32_t* tokens, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(scores && tokens && B >= 1 && V >= 1, "bad arguments");
    TTS_REQUIRE(temperature && top_k && top_p && sample && row_seed, "missing per-row settings");
    TTS_REQUIRE((ids == nullptr) == (counts == nullptr), "a list needs ids and counts");
    SampleArgs a;
    a.logits = scores;
    a.row_temp = temperature; a.row_top_k = top_k; a.row_top_p = top_p; a.row_sample = sample; a.row_stride = 1;
    a.row_seed = (const unsigned long long*)row_seed; a.step0 = step;
    a.probs = probs; a.tokens = tokens;
    if (ids) {
      TTS_REQUIRE(cap >= 1, "bad arguments");
      a.list_idx = ids; a.list_cnt = const_cast<int32_t*>(counts);  // (list_clear 0: only read)
      a.ldl = cap; a.V = cap; a.vocab = V;
      launch_sample_list_rows(a, B, (hipStream_t)stream);
    } else {
      a.ldl = V; a.V = V;
      const bool parts = part_max != nullptr && nparts > 0;
      a.part_val = parts ? part_max : nullptr; a.part_idx = parts ? part_idx : nullptr;
      a.nparts = parts ? nparts : 0; a.part_stride = nparts;
      launch_sample_rows(a, B, (hipStream_t)stream);
    }
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_rmsnorm(const void* x, const void* w, float eps, void* y, int32_t M, int32_t K,
                          void* stream) {
  return guarded([&] {
    TTS_REQUIRE(x && w && y && K % 8 == 0, "bad argument");
    launch_rmsnorm((const bf16_t*)x, K, (const bf16_t*)w, eps, (bf16_t*)y, K, M, K,
                   (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

// What the attention kernels support (lm_attn.hip): checked before any launch.
static AttnArgs attn_op_args(const void* qkv, int32_t ld_qkv, int32_t n_slots, void* kcache, void* vtcache,
                             int32_t max_seq, const void* rope_cos, const void* rope_sin, int32_t H,
                             int32_t KVH, int32_t D, float scale, void* out) {
  TTS_REQUIRE(kcache && vtcache && rope_cos && rope_sin && out, "null argument");
  TTS_REQUIRE(D == 64 || D == 128, "head dim must be 64 or 128");
  TTS_REQUIRE(KVH >= 1 && H == 4 * KVH, "num_heads must be 4 * num_kv_heads");
  TTS_REQUIRE(max_seq >= 64 && max_seq % 64 == 0, "max_seq must be a multiple of 64");
  TTS_REQUIRE((long long)max_seq * D < (1ll << 31), "max_seq * head_dim must be below 2^31");
  TTS_REQUIRE(n_slots >= 1, "n_slots must be >= 1");
  TTS_REQUIRE(ld_qkv >= (H + 2 * KVH) * D && ld_qkv % 8 == 0, "ld_qkv below (H + 2 KVH) D or not a multiple of 8");
  AttnArgs a;
  a.qkv = (const bf16_t*)qkv; a.ld_qkv = ld_qkv;
  a.kcache = (bf16_t*)kcache; a.vtcache = (bf16_t*)vtcache; a.max_seq = max_seq;
  a.rope_cos = (const bf16_t*)rope_cos; a.rope_sin = (const bf16_t*)rope_sin;
  a.H = H; a.KVH = KVH; a.D = D; a.scale = scale;
  a.out = (bf16_t*)out;
  return a;
}

// every row's slot inside the cache and used once, every position inside the stride
static void attn_op_check_rows(const std::vector<int>& slot, const std::vector<int>& last_pos, int n_slots,
                               int max_seq) {
  std::vector<char> used(n_slots, 0);
  for (size_t i = 0; i < slot.size(); ++i) {
    TTS_REQUIRE(slot[i] >= 0 && slot[i] < n_slots, "slot out of range");
    TTS_REQUIRE(!used[slot[i]], "a slot appears twice");
    used[slot[i]] = 1;
    TTS_REQUIRE(last_pos[i] >= 0 && last_pos[i] < max_seq, "position out of range (>= max_seq)");
  }
}

tts_status tts_op_attn_prefill(const void* qkv, int32_t ld_qkv, const int32_t* seq_slot, const int32_t* seq_pos0,
                               const int32_t* seq_len, int32_t n_seq, int32_t n_slots, void* kcache,
                               void* vtcache, int32_t max_seq, const void* rope_cos, const void* rope_sin,
                               int32_t H, int32_t KVH, int32_t D, float scale, void* q_rot, void* out,
                               void* stream) {
  return guarded([&] {
    TTS_REQUIRE(qkv && seq_slot && seq_pos0 && seq_len && q_rot && n_seq >= 1, "null argument");
    AttnArgs a = attn_op_args(qkv, ld_qkv, n_slots, kcache, vtcache, max_seq, rope_cos, rope_sin, H, KVH, D,
                              scale, out);
    TTS_REQUIRE(KVH <= 8, "prefill: at most 8 kv heads");
    std::vector<int> slot, pos, blk, sslot(seq_slot, seq_slot + n_seq), slast(n_seq);
    int rows = 0;
    for (int b = 0; b < n_seq; ++b) {
      TTS_REQUIRE(seq_len[b] >= 1 && seq_pos0[b] >= 0 && seq_len[b] <= max_seq, "bad sequence length / first position");
      slast[b] = seq_pos0[b] + seq_len[b] - 1;
    }
    attn_op_check_rows(sslot, slast, n_slots, max_seq);
    for (int b = 0; b < n_seq; ++b) {
      prefill_seq_rows(seq_slot[b], seq_pos0[b], seq_len[b], rows, slot, pos, blk);
      rows += seq_len[b];
    }
    hipStream_t s = (hipStream_t)stream;
    int* dev = nullptr;  // row_slot | row_pos | blocks (16-byte aligned: rows rounded up to 4)
    const size_t r4 = ((size_t)rows + 3) / 4 * 4;
    HIP_CHECK(hipMallocAsync((void**)&dev, (2 * r4 + blk.size()) * 4, s));
    HIP_CHECK(hipMemcpyAsync(dev, slot.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dev + r4, pos.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dev + 2 * r4, blk.data(), blk.size() * 4, hipMemcpyHostToDevice, s));
    a.rows = rows; a.row_slot = dev; a.row_pos = dev + r4;
    a.blocks = (const int4*)(dev + 2 * r4); a.nblocks = (int)blk.size() / 4;
    a.q_rot = (bf16_t*)q_rot;
    launch_rope_append(a, s);
    launch_attn_prefill(a, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipFreeAsync(dev, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the host vectors above are the copies' sources)
  });
}

tts_status tts_op_attn_decode(const void* qkv, const float* qkv_part, int32_t qkv_nsl, int32_t ld_qkv,
                              int32_t rows, const int32_t* row_slot, const int32_t* row_pos, int32_t n_slots,
                              void* kcache, void* vtcache, int32_t max_seq, const void* rope_cos,
                              const void* rope_sin, int32_t H, int32_t KVH, int32_t D, float scale, void* out,
                              void* stream) {
  return guarded([&] {
    TTS_REQUIRE(row_slot && row_pos && rows >= 1, "null argument");
    TTS_REQUIRE((qkv != nullptr) != (qkv_part != nullptr), "exactly one of qkv and qkv_part");
    TTS_REQUIRE(!qkv_part || qkv_nsl >= 1, "qkv_part needs qkv_nsl >= 1");
    AttnArgs a = attn_op_args(qkv, ld_qkv, n_slots, kcache, vtcache, max_seq, rope_cos, rope_sin, H, KVH, D,
                              scale, out);
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> slot(rows), pos(rows);
    HIP_CHECK(hipMemcpyAsync(slot.data(), row_slot, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(pos.data(), row_pos, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    attn_op_check_rows(slot, pos, n_slots, max_seq);
    a.rows = rows; a.row_slot = row_slot; a.row_pos = row_pos;
    a.qkv_part = qkv_part; a.qkv_nsl = qkv_part ? qkv_nsl : 0;
    launch_attn_decode_step(a, s);
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_gemm_f32(const float* A, int32_t M, int32_t K, int32_t lda, const float* B,
                           int32_t N, const float* bias, float* C, int32_t ldc,
                           const float* resid, int32_t act, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "bad argument");
    GemmF32Args g;
    g.A = A; g.M = M; g.K = K; g.lda = lda; g.B = B; g.N = N; g.bias = bias;
    g.C = C; g.ldc = ldc; g.resid = resid; g.act = act;
    launch_gemm_f32(g, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_split_planes(const float* x, uint16_t* planes, int64_t n, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(x && planes && n >= 1, "null argument");
    launch_split_planes(x, planes, (long long)n, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
  });
}

tts_status tts_op_gemm_planes(const float* A, const uint16_t* Ap, int64_t ap_plane, int32_t M, int32_t K, int32_t lda,
                              const float* B, const uint16_t* Bp, int32_t N, const float* bias, float* C,
                              uint16_t* Cp, int64_t cp_plane, int32_t ldc, const float* resid, int32_t act,
                              int32_t form, void* stream) {
  return guarded([&] {
    TTS_REQUIRE(M >= 1 && N >= 1 && K >= 1, "bad shape: M, N, K >= 1");
    TTS_REQUIRE(A || Ap, "planes missing: neither A nor Ap");
    TTS_REQUIRE(B || Bp, "planes missing: neither B nor Bp");
    TTS_REQUIRE(C || Cp, "no output: neither C nor Cp");
    TTS_REQUIRE(ldc >= N && lda >= 1, "ldc < N or lda < 1");
    TTS_REQUIRE(act == 0 || act == 1, "act is 0 or 1");
    // the kernels' 16-byte loads: fp32 rows in float4, plane rows in 8 bf16
    TTS_REQUIRE(!A || (lda % 4 == 0 && ((size_t)A & 15) == 0), "A: lda % 4 != 0 or an unaligned base");
    TTS_REQUIRE(!Ap || (lda % 8 == 0 && ap_plane % 8 == 0 && ((size_t)Ap & 15) == 0),
                "Ap: lda % 8 != 0, ap_plane % 8 != 0 or an unaligned base");
    TTS_REQUIRE(K % 4 == 0 && ((size_t)B & 15) == 0 && ((size_t)Bp & 15) == 0, "B / Bp: K % 4 != 0 or an unaligned base");
    TTS_REQUIRE(!Bp || K % 8 == 0, "Bp: K % 8 != 0");
    GemmF32Args g;
    g.A = A; g.Ap = Ap; g.ap_plane = ap_plane; g.M = M; g.K = K; g.lda = lda;
    g.B = B; g.Bp = Bp; g.N = N; g.bias = bias;
    g.C = C; g.Cp = Cp; g.cp_plane = cp_plane; g.ldc = ldc; g.resid = resid; g.act = act;
    hipStream_t s = (hipStream_t)stream;
    if (form == -1) {  // the engine's wrappers: planes-only A is gemm_p's call, else gemm's
      if (!A) {
        TTS_REQUIRE(Bp, "planes missing: Ap without Bp");
        launch_gemm_x3p(g, s);
      } else {
        TTS_REQUIRE(B, "fp32 A needs fp32 B (Bp beside it is optional)");
        TTS_REQUIRE(K % 16 == 0, "K % 16 != 0");
        launch_gemm_f32(g, s);
      }
    } else if (form >= 0 && form < 0x80) {
      TTS_REQUIRE(Ap && Bp, "planes missing: the x3p forms read Ap and Bp");
      const int sched = (form >> 3) & 3;
      TTS_REQUIRE(sched != 3, "unknown form");
      launch_gemm_x3p_form(g, form & 7, sched == 2 ? -1 : sched, (form & 0x20) != 0, (form & 0x40) != 0, s);
    } else if (form >= 0x100 && form < 0x100 + kF32_64x64) {
      launch_gemm_f32_form(g, form - 0x100, s);
    } else if (form >= 0x200 && form < 0x200 + (kGemmForms - kF32_64x64)) {
      launch_gemm_f32_form(g, kF32_64x64 + form - 0x200, s);
    } else {
      TTS_REQUIRE(false, "unknown form");
    }
    HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
