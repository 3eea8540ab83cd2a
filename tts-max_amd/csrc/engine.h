// engine.h — the engine object behind the C ABI (one GPU, one stream, owned buffers).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/tts_mi355x.h"
#include "env.h"
#include "lm_kernels.h"

namespace tts {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIP_CHECK(expr)                                                                    \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      throw ::tts::Error(TTS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) +    \
                                        " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
  } while (0)
#define TTS_REQUIRE(cond, msg)                                    \
  do {                                                            \
    if (!(cond)) throw ::tts::Error(TTS_E_INVALID, std::string(msg)); \
  } while (0)

// Device allocation owned by the engine.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void alloc(size_t n) {
    release();
    if (n == 0) n = 16;
    if (hipMalloc(&p, n) != hipSuccess) {
      p = nullptr;
      throw Error(TTS_E_OOM, "hipMalloc failed for " + std::to_string(n) + " bytes");
    }
    bytes = n;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T> T* as() const { return (T*)p; }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

struct LmLayer {
  bf16_t* ln1;   // [hidden]
  bf16_t* ln2;
  bf16_t* wqkv;  // tiled [(H+2KVH)*D][hidden]
  bf16_t* wo;    // tiled [hidden][H*D]
  bf16_t* wgu;   // tiled, gate/up n-tiles interleaved [2*ffn][hidden]
  bf16_t* wd;    // tiled [hidden][ffn]
};

struct LmModel {
  tts_lm_config cfg{};
  bool loaded = false;
  DevBuf weights;       // one slab for every tiled matrix + norms
  DevBuf embed_rows;    // row-major embedding [V][hidden] (token gather)
  DevBuf rope;          // cos | sin  [max_seq][D] bf16 each
  std::vector<LmLayer> layers;
  bf16_t* final_norm = nullptr;
  bf16_t* lm_head = nullptr;  // tiled [V][hidden]
  // the greedy lm_head's int8 screen (lm_head_screen.hip): codes in the screen's block layout,
  // per-column {scale, |W - Wh|, |W|, |Wh|}; head_grid = the screen's launch grid (0: none)
  DevBuf head_q, head_c;
  int head_grid = 0;
  std::vector<int> id_to_code;  // host LUT (optional)
  int qkv_n() const { return (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim; }
};

// What the captured decode step bakes in as kernel arguments: a generation whose key differs
// needs a recapture.  (The sampling keys are per-row device values, LmWork::row_seed: a new
// seed needs none.)  temp / top_k / top_p count only for a sampled step (-1 when greedy).
// per_row (the per-request slot batch): the settings are per-row device values too
// (LmWork::row_par) and the other settings fields stay neutral, so admitting a request with new
// settings needs no recapture; dense = the step takes the full lm_head + the dense sampler instead
// of the screen's per-row top-k form (a resident request's top_k is above what the screen covers).
struct StepKey {
  int batch = -1;
  float pen = -1.f;
  int eos = -2, min_new = -1;
  int sample = -1, top_k = -1;
  float temp = -1.f, top_p = -1.f;
  float freq = 0.f;
  int per_row = 0, dense = 0;
  StepKey() = default;
  static StepKey rows(int B, bool dense) {
    StepKey k;
    k.batch = B; k.per_row = 1; k.dense = dense ? 1 : 0;
    return k;
  }
  StepKey(int B, const tts_gen_params& p)
      : batch(B), pen(p.repetition_penalty), eos(p.eos_token_id), min_new(p.min_new_tokens),
        sample(p.do_sample), top_k(p.do_sample ? p.top_k : -1), temp(p.do_sample ? p.temperature : -1.f),
        top_p(p.do_sample ? p.top_p : -1.f), freq(p.frequency_penalty) {}
  bool operator==(const StepKey& o) const {
    return batch == o.batch && pen == o.pen && eos == o.eos && min_new == o.min_new && sample == o.sample &&
           top_k == o.top_k && temp == o.temp && top_p == o.top_p && freq == o.freq && per_row == o.per_row &&
           dense == o.dense;
  }
};

// LmWork::ferr: ints the kernels raise and read_device_flags (lm_generate.cpp) reports
enum {
  FERR_GRANULE_TIMEOUT = 0,  // fused QKV+attention: a granule wait timed out
  FERR_SCREEN_CHECK = 1,     // screened lm_head, check mode: a score outside its bound (the launch's `err`)
  FERR_SCREEN_DIAG = 3,      // TTS_HEAD_SCREEN_DIAG=2: units recomputed (the launch counts at err[2])
  FERR_SLOTS = 4
};

struct LmWork {
  int cap_rows = 0;    // activation rows (prefill rows and decode batch)
  int cap_batch = 0;
  DevBuf kv;           // per layer: K [slots][KVH][kv_stride][D], V^T [slots][KVH][D][kv_stride]
  int kv_stride = 0;   // positions per (slot, kv head) strip: max_seq_len rounded up to 64
  DevBuf x, xn, qkv, attn_out, act, q_rot, last_x;  // activations
  DevBuf blocks;                                    // prefill query blocks (int4, lm_attn.hip)
  int nblocks = 0;
  DevBuf gran, ferr;                                // fused QKV+attention: granules [QKV/2] u64, error flag
  DevBuf epoch;                                     // decode-step counter (u32; the screened head's step keys)
  DevBuf lpart_v, lpart_i;                          // lm_head argmax partials
  DevBuf hub, hlb;                                  // screened head: check-mode score bounds [B][V], per-row max lower bound (u64)
  DevBuf hslot, hcv, hci, hcn, hlo;                 // sampled screened head: workgroup slots (u64), candidate scores / ids [16][V], counts, check-mode lower bounds
  DevBuf hxq, hxs;                                  // screened head at 17..32 rows: the rows quantised [2B][hidden] i8, their stats
  DevBuf kpart;                                     // K-sliced GEMM fp32 partials [kc][rows][N]
  DevBuf ppart;                                     // prefill GEMM fp32 partials [chunks][rows][N] (lm_pgemm.hip)
  DevBuf slogits;                                   // sampling: processed fp32 logits [B][V]
  DevBuf counts;                                    // vLLM frequency penalty: new-token counts [B][V] u16
  DevBuf row_slot, row_pos, row_idx;                // prefill row descriptors
  DevBuf st_int;                                    // step-state ints
  DevBuf row_seed;                                  // [B] u64 sampling key of each row (graph-invariant)
  DevBuf row_par;                                   // [cap_batch] RowParams: the per-request slot batch's settings table
  DevBuf seen;                                      // [B][V/32]
  DevBuf out_ids;                                   // [B][max_new]
  int out_cap = 0;
  hipGraphExec_t graph = nullptr;
  StepKey step_key;  // what `graph` was captured with
  int* h_active = nullptr;  // pinned host copy of n_active (ring of 2)
};

struct Codec;         // codec_engine.cpp
struct AudioEncoder;  // codec_encoder.cpp

struct Engine {
  int device = 0;
  int num_cu = 256;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {};
  LmModel lm;
  LmWork w;
  Codec* codec = nullptr;
  AudioEncoder* encoder = nullptr;
  float t_prefill_ms = 0.f, t_decode_ms = 0.f;
  int decode_steps = 0;
  // an open generation (tts_generate_begin .. tts_generate_read): state lives on the device
  struct Gen {
    bool open = false;
    int B = 0, max_new = 0, launched = 0, polls = 0;
    bool finished = false;
    hipStream_t s = nullptr;
  } gen;
  // continuous batching (tts_slots_*): S persistent rows, sequences admitted / retired
  // between decode chunks
  struct Slots {
    bool open = false;
    int S = 0;
    tts_gen_params gp{};
    unsigned long long next_req = 0;  // default per-request sampling keys
    // per-request batch (tts_slots_open_per_request): every row's settings in LmWork::row_par (gp =
    // the defaults); dense: a request above the screen's top_k bound was admitted (until reopened)
    bool per_row = false, dense = false;
    int max_top_k = 1;  // the largest top_k admitted so far (the screen's host check)
    std::vector<int> busy;  // 1 while a sequence owns the slot (until released)
    hipStream_t s = nullptr;
  } slots;
  ~Engine();
};

hipStream_t pick_stream(Engine* e, void* s);
void lm_load(Engine* e, const tts_lm_config* cfg, const tts_tensor_desc* t, int n);
void lm_generate(Engine* e, const tts_gen_params* p, const int32_t* ids, const int32_t* lens,
                 int B, int32_t* out_ids, int out_stride, int32_t* out_lens, hipStream_t s);
// the same loop in pieces (streaming): begin = prefill + first token; continue = up to
// n_steps more decode steps (returns 1 when every row has stopped); read = ids so far
void lm_gen_begin(Engine* e, const tts_gen_params* p, const int32_t* ids, const int32_t* lens, int B,
                  hipStream_t s);
int lm_gen_continue(Engine* e, int n_steps);
void lm_gen_read(Engine* e, int32_t* out_ids, int out_stride, int32_t* out_lens);
void lm_slots_open(Engine* e, const tts_gen_params* p, int S, hipStream_t s, bool per_request = false);
// rp: the request's own settings (a per-request batch only), or nullptr: the batch's
void lm_slots_add(Engine* e, int slot, const int32_t* prompt, int len, int max_new, const uint64_t* seed,
                  const tts_gen_params* rp = nullptr);
int lm_slots_step(Engine* e, int n_steps);
void lm_slots_read(Engine* e, int slot, int32_t* out_ids, int cap, int32_t* n_out, int32_t* finished);
void lm_slots_release(Engine* e, int slot);
void lm_score(Engine* e, const int32_t* ids, const int32_t* lens, int B, int n_last,
              float* logits, hipStream_t s);
void lm_score_decode(Engine* e, const int32_t* ids, const int32_t* lens, int B, int n_last,
                     const int32_t* gidx, int k, float* out, hipStream_t s);
void lm_bench_kernel(Engine* e, int which, int rows, int ctx, int iters, float* avg_ms,
                     double* bytes);
// top_k > 0: a sampled step; per_row: the per-request batch's step (top_k = its largest admitted top_k)
std::string lm_step_plan(const tts_lm_config& c, int rows, int num_cu, int top_k = 0, bool per_row = false);

// upload a named tensor to device memory as bf16 (convert from f32 if needed)
void upload_bf16(const tts_tensor_desc& d, bf16_t* dst, hipStream_t s, DevBuf& staging);
int64_t numel(const tts_tensor_desc& d);

void codec_load(Engine* e, const tts_codec_config* cfg, const tts_tensor_desc* t, int n);
void codec_decode(Engine* e, const int32_t* codes, const int32_t* lens, int B, float* wav,
                  int wav_is_device, int64_t* wav_lens, hipStream_t s);
int codec_samples_per_code(Engine* e);
// the prompt-audio encoder (codec_encoder.cpp)
void encoder_load(Engine* e, const tts_tensor_desc* t, int n);
int encoder_encode(Engine* e, const float* wav, int n, const float* w2v, int T_w2v, int32_t* codes, int cap,
                   float* pre, const float* feats = nullptr);
void encoder_destroy(AudioEncoder* a);
void codec_destroy(Codec* c);

}  // namespace tts
