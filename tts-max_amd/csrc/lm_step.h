// lm_step.h — one SpeechLM transformer step as a sequence of launches: the step composition
// (Ctx, defined in lm_step.cpp), the step-state layout, and what the runtime's files share.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cstdio>

#include "engine.h"

namespace tts {

constexpr int kPrefillChunk = 64;   // rows per decode GEMM launch set (MFMA A-tiles of 16); more rows: the tile GEMMs
constexpr int kMaxPrefillRows = 8192;

size_t kpart_bytes(const tts_lm_config& c);                // lm_load.cpp: LmWork::kpart's size
size_t ppart_bytes(const tts_lm_config& c);                // lm_load.cpp: LmWork::ppart's size
int head_screen_grid(const tts_lm_config& c, int num_cu);  // lm_load.cpp: the int8 screen's grid (0: no screen)
bool head_screen_check();                                  // lm_step.cpp: TTS_HEAD_SCREEN_CHECK
unsigned long long* stamp_buf();                           // lm_debug.cpp: null but in the stamps build
void read_device_flags(Engine* e, hipStream_t s);          // lm_generate.cpp: throws what LmWork::ferr holds

// LmWork::st_int: ST_N_ACTIVE arrays of B ints in this order, then the active-row count
enum { ST_TOKENS, ST_POS, ST_GEN_COUNT, ST_LIMIT, ST_DONE, ST_EOS_MASK, ST_N_ACTIVE };
inline int st_at(int array, int B, int b) { return array * B + b; }
inline std::vector<int> st_zeros(int B) { return std::vector<int>(st_at(ST_N_ACTIVE, B, B) + 1, 0); }
// row `slot` of a step state as a batch of 1 (n_active and epoch stay the batch's)
StepState step_state_row(const StepState& st, int slot);

struct Ctx {
  Engine* e;
  hipStream_t s;
  const tts_lm_config& c;
  LmModel& M;
  LmWork& w;
  Ctx(Engine* e_, hipStream_t s_) : e(e_), s(s_), c(e_->lm.cfg), M(e_->lm), w(e_->w) {}
  int QKV() const { return M.qkv_n(); }

  // Invariant: when non-null, w.xn holds RMSNorm(w.x, pending_norm) for every row of the pass (a
  // residual launch's combine wrote it beside w.x), so a GEMM over w.x with that norm weight
  // reads w.xn and skips its norm.  Any launch that rewrites w.x clears or replaces it.
  const bf16_t* pending_norm = nullptr;

  // ---- the layer's four projections and the lm_head over `rows` rows
  // w.qkv = RMSNorm(w.x, ln1) . Wqkv^T.  defer_combine (17..32 decode rows): the K-sliced form may
  // leave its fp32 partials in w.kpart for the decode attention to sum; returns whether it did
  bool qkv_proj(int rows, const LmLayer& ly, bool defer_combine = false) {
    Gemm g{w.x.as<bf16_t>(), rows, c.hidden_size, ly.wqkv, QKV(), EPI_STORE};
    g.out = w.qkv.as<bf16_t>(); g.ldo = QKV(); g.normw = ly.ln1; g.defer_combine = defer_combine;
    return gemm(g);
  }
  // ... with the decode attention (and o_proj) in the same launch (fused_attn_args)
  void qkv_attn_proj(int rows, const LmLayer& ly, const WgemmArgs& fused) {
    Gemm g{w.x.as<bf16_t>(), rows, c.hidden_size, ly.wqkv, QKV(), EPI_STORE};
    g.out = w.qkv.as<bf16_t>(); g.ldo = QKV(); g.normw = ly.ln1; g.extra = &fused;
    gemm(g);
  }
  // w.x += w.attn_out . Wo^T; next_norm: the combine may also leave RMSNorm(w.x, next_norm) in w.xn
  void o_proj(int rows, const LmLayer& ly, const bf16_t* next_norm = nullptr) {
    Gemm g{w.attn_out.as<bf16_t>(), rows, c.num_heads * c.head_dim, ly.wo, c.hidden_size, EPI_RESID};
    g.ldo = c.hidden_size; g.resid = w.x.as<bf16_t>(); g.next_norm = next_norm;
    gemm(g);
  }
  void gate_up(int rows, const LmLayer& ly) {  // w.act = SwiGLU(RMSNorm(w.x, ln2) . Wgu^T)
    Gemm g{w.x.as<bf16_t>(), rows, c.hidden_size, ly.wgu, 2 * c.intermediate_size, EPI_SWIGLU};
    g.out = w.act.as<bf16_t>(); g.ldo = c.intermediate_size; g.normw = ly.ln2;
    gemm(g);
  }
  void down_proj(int rows, const LmLayer& ly, const bf16_t* next_norm = nullptr) {  // w.x += w.act . Wd^T
    Gemm g{w.act.as<bf16_t>(), rows, c.intermediate_size, ly.wd, c.hidden_size, EPI_RESID};
    g.ldo = c.hidden_size; g.resid = w.x.as<bf16_t>(); g.next_norm = next_norm;
    gemm(g);
  }
  // lm_head over RMSNorm(x, final norm): the processing epilogue + argmax partials, or plain logits
  // (tile_head: more than kPrefillChunk rows may run as the tile head, the wide decode step's form)
  void lm_head_pick(const bf16_t* x, int rows, const WgemmArgs& epilogue, int epi = EPI_LOGITS, bool tile_head = false) {
    Gemm g{x, rows, c.hidden_size, M.lm_head, c.vocab_size, epi};
    g.normw = M.final_norm; g.extra = &epilogue; g.tile_head = tile_head;
    gemm(g);
  }
  void lm_head_logits(const bf16_t* x, int rows, bf16_t* out) {  // out: bf16 [rows][V]
    Gemm g{x, rows, c.hidden_size, M.lm_head, c.vocab_size, EPI_STORE};
    g.out = out; g.ldo = c.vocab_size; g.normw = M.final_norm;
    gemm(g);
  }

  AttnArgs attn_args(int layer, int rows, const int* slot, const int* pos, bool qkv_part = false);
  bool fused_attn_ok(int rows, bool decode) const;
  WgemmArgs fused_attn_args(const AttnArgs& a, int layer, bool with_oproj = false);
  // the warm role riding that launch at one row: wgu = the layer's gate/up weights, first_block =
  // the grid index of the first warm workgroup (all-zero: no warm role)
  WarmArgs warm_args(const bf16_t* wgu, int first_block) const;
  bool gate_up_ring4() const;  // the one-row gate/up launch behind it on the four-stage ring (TTS_GU_RING)
  bool fused_oproj_ok() const;
  bool fused_oproj_rows_ok(int rows) const;
  void layers(int rows, const int* slot, const int* pos, bool decode);  // one stack pass over w.x

  StepState state(int B, int eos, int min_new);
  WgemmArgs head_epilogue_args(const StepState& st, const tts_gen_params& gp);  // lm_head_pick's
  // the sampler's: over the dense logits (nparts workgroup maxima a row) or the screen's lists
  SampleArgs sample_args(const StepState& st, const tts_gen_params& gp, bool lists, int nparts = 0);
  // step: the decode step's pick (65..256 rows: the tile head); else a first token from prefilled
  // rows, which takes the decode head's K order at every B, as a slot admission's batch of 1 does
  void head_and_pick(const bf16_t* xin, int B, const StepState& st, const tts_gen_params& gp, bool step = false);
  int head_parts(int B, int epi, bool step) const;
  // the per-request batch's pick (st.par, st.counts set): the screen's per-row top-k form + the
  // per-row list sampler where the rows and max_top_k fit it and !dense, else the per-row full head
  // + the per-row dense sampler
  bool rows_screen_ok(int B, int max_top_k) const;
  void head_and_pick_rows(const bf16_t* xin, int B, const StepState& st, bool dense, int max_top_k);
  void screened_sample(const bf16_t* xin, int B, const StepState& st, const tts_gen_params& gp);
  // (par: the per-row variant of the top-k mode, top_k = the batch's largest)
  int screened_head_parts(const bf16_t* xin, int B, const StepState& st, const tts_gen_params& gp, int top_k = 0,
                          const RowParams* par = nullptr);

  // Prefill nb whole sequences (ids concatenated; KV slots slot_base..) in one pass: row setup +
  // layers, and (gather_row >= 0) their last rows into w.last_x from that row on.  Returns each
  // sequence's last row in w.x.
  std::vector<int> prefill_group(const int32_t* ids, const int32_t* lens, int nb, int slot_base, int gather_row = -1);
  // ... every sequence (b: lens[b] ids at ids + start[b]), in groups that fit the prefill workspace
  void prefill_all(const int32_t* ids, const std::vector<int>& start, const std::vector<int>& lens, bool gather_last,
                   const char* what);
  void upload_identity_slots(int B) {  // w.row_slot = 0..B-1: the decode phase's rows are their slots
    std::vector<int> ident(B);
    for (int b = 0; b < B; ++b) ident[b] = b;
    HIP_CHECK(hipMemcpyAsync(w.row_slot.p, ident.data(), B * 4, hipMemcpyHostToDevice, s));
  }

 private:
  struct Gemm {  // out[rows][ldo] = epi(norm?(x[rows][K]) . W^T), W tiled [N][K]
    const bf16_t* x;
    int rows, K;
    const bf16_t* W;
    int N, epi;
    bf16_t* out = nullptr;
    int ldo = 0;
    const bf16_t* normw = nullptr;      // RMSNorm prologue
    bf16_t* resid = nullptr;            // EPI_RESID: the residual stream
    const WgemmArgs* extra = nullptr;   // the lm_head epilogue's, or the fused attention's, operands
    const bf16_t* next_norm = nullptr;  // EPI_RESID: the combine may normalise into w.xn
    bool defer_combine = false;         // EPI_STORE, 17..32 rows: partials may stay in w.kpart
    bool tile_head = false;             // EPI_LOGITS*, > kPrefillChunk rows: the tile head (TTS_WIDE_HEAD)
  };
  bool gemm(const Gemm& g);  // true: the partials were left in w.kpart (defer_combine)
  bool norm_once_ok(int rows) const;
  void finalize(int nparts, int B, const StepState& st) {  // the pick's bookkeeping + the next embedding -> w.x
    launch_finalize_greedy(w.lpart_v.as<float>(), w.lpart_i.as<int>(), LOGITS_MAX_PARTS, nparts, st, B,
                           M.embed_rows.as<bf16_t>(), w.x.as<bf16_t>(), c.hidden_size, s);
  }
};

}  // namespace tts
