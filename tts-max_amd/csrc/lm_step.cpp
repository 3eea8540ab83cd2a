// lm_step.cpp — the composition of one SpeechLM transformer step (lm_step.h): which kernel runs
// with which arguments, for prefill rows and for the decode step, and the dry-run step plan.
#include "lm_step.h"

namespace tts {

// The screened lm_head's workgroups wait for every workgroup's bounds before flagging their units (the
// exact candidate set; TTS_HEAD_SCREEN_WAIT=0: never, 1: always, n > 1: from n rows; unset: greedy
// steps from 2 rows — one row: 69 vs 73 us, 8 rows: 79 vs 96 us without,
// profiles/r6w_ab_head_wait_* — and sampled steps always: their threshold is the k-th largest of
// the workgroups' slots, and a workgroup that sees fewer than k of them recomputes all of its
// units).  Same bits either way: a lower bound only flags more units
static bool head_screen_wait(int rows, bool sampled = false) {
  static const int v = env_int("TTS_HEAD_SCREEN_WAIT", -1);
  if (v < 0) return sampled || rows >= 2;
  return v == 1 || (v > 1 && rows >= v);
}
// TTS_HEAD_SCREEN_CHECK=1: every unit recomputed and each exact score checked against its bound
// (greedy: the upper one, which the argmax depends on; sampled: both)
bool head_screen_check() { static const bool v = env_set("TTS_HEAD_SCREEN_CHECK"); return v; }

// Decode attention of a one-row step fused into the QKV launch (lm_gemm_kernel.h,
// fattn_consumer): default on; TTS_FUSED_ATTN=0 keeps the separate attention launch.
static bool use_fused_attn() { static const bool v = env_on("TTS_FUSED_ATTN"); return v; }
// ... and o_proj fused behind that attention (lm_gemm_kernel.h fused_oproj): default on;
// TTS_FUSED_OPROJ=0 keeps the separate o_proj launch.
static bool use_fused_oproj() { static const bool v = env_on("TTS_FUSED_OPROJ"); return v; }

// 17..32 rows: the decode attention sums the K-sliced QKV partials (no combine launch);
// TTS_QKV_DEFER=0 keeps the combine launch (same sums in the same order: the same bits)
static bool use_qkv_defer() { static const bool v = env_on("TTS_QKV_DEFER"); return v; }
static bool use_kslice32() { static const bool v = env_on("TTS_KSLICE32"); return v; }
// ... and at 2..16 rows, o_proj fused behind the attention of the QKV launch (its own
// workgroups after the attention's): default on; TTS_FUSED_OPROJ_ROWS=0 keeps the launch
static bool use_fused_oproj_rows() { static const bool v = env_on("TTS_FUSED_OPROJ_ROWS"); return v; }

// The lm_head of a 65..256-row decode step as one tile launch (head_tile_kernel, lm_pgemm.hip):
// default on; TTS_WIDE_HEAD=0 runs it as the 32-row decode head in chunks (the head streamed once
// per chunk; the decode stream's K order instead of the canonical chunks)
static bool use_wide_head() { static const bool v = env_on("TTS_WIDE_HEAD"); return v; }

StepState step_state_row(const StepState& st, int slot) {
  StepState one = st;
  one.tokens += slot; one.pos += slot; one.gen_count += slot; one.limit += slot;
  one.done += slot; one.eos_mask += slot; one.row_seed += slot;
  if (one.par) one.par += slot;
  one.seen += (size_t)slot * st.seen_stride;
  one.out_ids += (size_t)slot * st.out_stride;
  if (one.counts) one.counts += (size_t)slot * st.seen_stride * 32;
  return one;
}

// RMSNorm once per row by the producing launch (2..32 decode rows): the K-sliced down
// projection's combine (a per-row kernel already) normalises with the next norm weight;
// TTS_NORM_ONCE=0: every consuming workgroup normalises in its prologue
bool Ctx::norm_once_ok(int rows) const {
  static const bool on = env_on("TTS_NORM_ONCE");
  return on && rows >= 2 && rows <= 32 && c.hidden_size % 512 == 0 && c.hidden_size <= 8192;
}

// out = epi(x . W^T) over g.rows rows (chunked by 64), RMSNorm prologue if g.normw
bool Ctx::gemm(const Gemm& g) {
  const auto [x, rows, K, W, N, epi, out, ldo, normw, resid, logit_extra, next_norm, defer_combine, tile_head] = g;
  bool part_left = false;
  const bf16_t* ready = pending_norm;
  if (resid) pending_norm = nullptr;  // the residual stream changes below
  const bool have_x = x || dry_launches();  // (a dry run has no buffers)
  if (tile_head && rows > kPrefillChunk && have_x && logit_extra && use_wide_head() && head_tile_supported(rows, N, K)) {
    // the wide decode step's lm_head: every row in one tile launch with the pick's epilogue
    TTS_REQUIRE(normw != nullptr, "the tile lm_head reads normalised rows");
    if (!(normw == ready && x == w.x.as<bf16_t>()))
      launch_rmsnorm(x, K, normw, c.rms_norm_eps, w.xn.as<bf16_t>(), K, rows, K, s);
    const WgemmArgs& ex = *logit_extra;
    HeadTileArgs h;
    h.g.x = w.xn.as<bf16_t>(); h.g.M = rows; h.g.K = K; h.g.ldx = K;
    h.g.w = W; h.g.N = N;
    h.seen = ex.seen; h.seen_stride = ex.seen_stride; h.penalty = ex.penalty; h.eos_mask = ex.eos_mask;
    h.part_val = ex.part_val; h.part_idx = ex.part_idx; h.part_stride = ex.part_stride;
    h.logits_out = ex.logits_out; h.ldl = ex.ldl;
    h.counts = ex.counts; h.freq_penalty = ex.freq_penalty; h.row_par = ex.row_par;
    launch_head_tile(h, epi == EPI_LOGITS_ROWS, e->num_cu, s);
    return false;
  }
  if (rows > kPrefillChunk && have_x && pgemm_supported(rows, N, K, epi)) {
    // prefill: every prompt row of the batch in one LDS-staged MFMA launch
    const bf16_t* xin = x;
    if (normw) {
      // (rows a residual combine already normalised with this weight: none to redo)
      if (!(normw == ready && x == w.x.as<bf16_t>()))
        launch_rmsnorm(x, K, normw, c.rms_norm_eps, w.xn.as<bf16_t>(), K, rows, K, s);
      xin = w.xn.as<bf16_t>();
    }
    PgemmArgs a;
    a.x = xin; a.M = rows; a.K = K; a.ldx = K;
    a.w = W; a.N = N;
    a.out = out; a.ldo = ldo; a.resid = resid;
    a.part = w.ppart.as<float>(); a.part_bytes = w.ppart.bytes;
    if (resid == w.x.as<bf16_t>() && ldo == c.hidden_size && next_norm) {
      a.next_norm = next_norm; a.eps = c.rms_norm_eps; a.xn = w.xn.as<bf16_t>();
    }
    if (launch_pgemm(a, epi, e->num_cu, s)) pending_norm = next_norm;
    return false;
  }
  // decode GEMV launches hold at most 32 rows (two m-tiles: the A rows fit LDS); 33..64
  // rows run as two launches (the weights stream twice, still far cheaper than A rows
  // read from global memory); so does the lm_head of more rows where the tile head does not run
  // (the first token of a 65..256-row generate; TTS_WIDE_HEAD=0)
  const int chunk = rows > 32 ? 32 : kPrefillChunk;
  for (int r0 = 0; r0 < rows; r0 += chunk) {
    const int m = std::min(chunk, rows - r0);
    WgemmPlan p = plan_wgemm(m, N, K, epi, e->num_cu);
    if (p.sliced && wgemm_part_elems(p, m, ldo) * 4 > w.kpart.bytes) {
      p.sliced = false;  // wide outputs (teacher-forced scoring over the vocabulary):
      p.a_lds = false;   // A rows from global memory instead of fp32 chunk partials
    }
    if (epi == EPI_SWIGLU && rows == 1 && gate_up_ring4()) p.ring = 4;
    const bf16_t* xin = x ? x + (size_t)r0 * K : nullptr;
    bool norm = normw != nullptr;
    // fused RMSNorm only where the rows sit in registers (<= 16 rows, the early prologue):
    // at 17..64 rows every workgroup would normalise every row again — one standalone
    // pass (same canonical order: identical bits) is cheaper, or none when the producer
    // already wrote the normalised rows
    // (by the batch's row count: every chunk of a 33..64-row batch takes the same path)
    if (norm && normw == ready && x == w.x.as<bf16_t>()) {
      xin = w.xn.as<bf16_t>() + (size_t)r0 * K;
      norm = false;
    } else if (norm && (!p.a_lds || p.sliced || K > 4096 || rows > 16)) {
      launch_rmsnorm(xin, K, normw, c.rms_norm_eps, w.xn.as<bf16_t>(), K, m, K, s);
      xin = w.xn.as<bf16_t>();
      norm = false;
    }
    // 17..32 rows of qkv / o_proj (kc = 1, K 2048): K split over 4 workgroups (each stages a
    // quarter of the A rows, 32 KiB instead of 128) + a combine: plain bf16 rows, or residual
    // add + the next RMSNorm (the gate/up prologue's norm) in one pass.  TTS_KSLICE32=0: off
    // (chosen by the batch's row count, not the chunk's: a 33..64-row batch runs two chunks,
    // and every row of a batch must take the same arithmetic)
    if (!norm && rows > 16 && m <= 32 && K == 2048 && !logit_extra &&
        (epi == EPI_STORE || epi == EPI_RESID) && use_kslice32() && p.sp.kc == 1 && p.sp.waves == 16 && p.sp.ksplit == 16 && p.sp.ku == 2 && p.sp.ng == 1 &&
        (size_t)4 * m * ldo * 4 <= w.kpart.bytes) {
      WgemmArgs a;
      a.x = xin; a.M = m; a.K = K / 4; a.ldx = K;
      a.w = W; a.N = N; a.ldo = ldo;
      a.ur = p.sp.ur(); a.kc = 1;
      a.part_out = w.kpart.as<float>();
      a.stamps = stamp_buf();
      launch_wgemm_kslice(a, N / 16, s);
      bf16_t* o = out ? out + (size_t)r0 * ldo : nullptr;
      bf16_t* rs = resid ? resid + (size_t)r0 * ldo : nullptr;
      if (epi == EPI_STORE && defer_combine) {  // the decode attention sums the partials
        part_left = true;
      } else if (epi == EPI_RESID && next_norm && rows <= 32) {
        launch_splitk_combine_norm(w.kpart.as<float>(), 4, m, N, ldo, rs, ldo, next_norm, c.rms_norm_eps,
                                   w.xn.as<bf16_t>() + (size_t)r0 * ldo, ldo, s);
        pending_norm = next_norm;
      } else {
        launch_splitk_combine(w.kpart.as<float>(), 4, m, N, ldo, o, rs, ldo, s);
      }
      continue;
    }
    WgemmArgs a;
    if (logit_extra) {
      a = *logit_extra;
      if (r0 > 0) {  // per-row operands of the lm_head epilogue start at row r0
        if (a.seen) a.seen += (size_t)r0 * a.seen_stride;
        if (a.eos_mask) a.eos_mask += r0;
        if (a.part_val) a.part_val += (size_t)r0 * a.part_stride;
        if (a.part_idx) a.part_idx += (size_t)r0 * a.part_stride;
        if (a.logits_out) a.logits_out += (size_t)r0 * a.ldl;
        if (a.counts) a.counts += (size_t)r0 * a.seen_stride * 32;
        if (a.row_par) a.row_par += r0;
      }
    }
    a.x = xin; a.M = m; a.K = K; a.ldx = K;
    a.w = W; a.N = N;
    a.stamps = stamp_buf();
    a.normw = normw; a.eps = c.rms_norm_eps;
    a.out = out ? out + (size_t)r0 * ldo : nullptr; a.ldo = ldo;
    a.resid = resid ? resid + (size_t)r0 * ldo : nullptr;
    if (p.sliced) a.part_out = w.kpart.as<float>();
    // the next RMSNorm once per row: in the K-sliced launch's combine (the combine is per row)
    const bool fuse_norm = p.sliced && epi == EPI_RESID && next_norm && (m > 16 || norm_once_ok(rows)) &&
                           rows <= 32 && N <= 8192;
    if (fuse_norm) {
      a.next_norm = next_norm;
      a.norm_out = w.xn.as<bf16_t>() + (size_t)r0 * ldo;
    }
    launch_wgemm(a, p, epi, norm, s);
    if (fuse_norm) pending_norm = next_norm;
  }
  return part_left;
}

AttnArgs Ctx::attn_args(int layer, int rows, const int* slot, const int* pos, bool qkv_part) {
  AttnArgs a;
  const int H = c.num_heads, KVH = c.num_kv_heads, D = c.head_dim;
  const size_t kv_layer = (size_t)c.max_batch * KVH * w.kv_stride * D;
  a.qkv = w.qkv.as<bf16_t>(); a.ld_qkv = QKV(); a.rows = rows;
  a.row_slot = slot; a.row_pos = pos;
  a.kcache = w.kv.as<bf16_t>() + (size_t)layer * 2 * kv_layer;
  a.vtcache = a.kcache + kv_layer;
  a.max_seq = w.kv_stride;
  a.rope_cos = M.rope.as<bf16_t>();
  a.rope_sin = a.rope_cos + (size_t)c.max_seq_len * D;
  a.H = H; a.KVH = KVH; a.D = D;
  a.scale = (float)(1.0 / sqrt((double)D));
  a.q_rot = w.q_rot.as<bf16_t>(); a.out = w.attn_out.as<bf16_t>();
  a.blocks = w.blocks.as<int4>(); a.nblocks = w.nblocks;
  a.stamps = stamp_buf();
  if (qkv_part) {  // (qkv_proj left its K-sliced partials in w.kpart: the decode attention sums them)
    a.qkv_part = w.kpart.as<float>();
    a.qkv_nsl = 4;
  }
  return a;
}

// The one-row decode step's QKV launch carries the attention (TTS-1 geometry: head dim 64);
// consecutive fused launches differ in (pos, layer)
bool Ctx::fused_attn_ok(int rows, bool decode) const {
  if (!decode || !use_fused_attn() || c.num_layers < 2 || c.num_layers > 64) return false;
  if (rows == 1) return c.head_dim == 64 && wgemm_fattn_ok(QKV(), c.hidden_size, e->num_cu);
  // 2..16 rows (TTS_FATTN_ROWS = the largest batch that fuses, 16 at most; 0: none): the
  // attention workgroups after the projection's (deadlock-free order)
  static const int max_rows = env_int("TTS_FATTN_ROWS", 16);
  return rows <= std::min(16, max_rows) && wgemm_fattn_rows_ok(rows, QKV(), c.hidden_size, c.head_dim, e->num_cu);
}
// The warm role of the one-row fused launch (lm_kernels.h WarmArgs): TTS_WARM_STAGES=<W> stages of
// the layer's gate/up stream (default 2 = 2 MiB per XCD; 0: no warm workgroups; 3 was slower
// than none: the reads outlast the attention and delay o_proj's hand-off, profiles/warm_ab.txt)
// read by TTS_WARM_WGS workgroups behind the o_proj ones.  TTS_WARM_XCD_DIST: the XCDs between
// block 0 of the fused launch and block 0 of the gate/up launch behind it as the dispatcher deals
// them (0 in every launch measured, profiles/warm_xcd_placement.txt).
// The one-row gate/up launch behind that fused launch runs on the four-stage ring its 4..32-row
// form has (launch_shape), so the two stages behind the warm ones stream from HBM while the A row
// lands; TTS_GU_RING=2 keeps the two-stage ring.  Same arithmetic order: same bits.
bool Ctx::gate_up_ring4() const {
  static const bool on = env_int("TTS_GU_RING", 4) != 2;
  return on && fused_attn_ok(1, true) && fused_oproj_ok();
}
WarmArgs Ctx::warm_args(const bf16_t* wgu, int first_block) const {
  static const int stages = env_int("TTS_WARM_STAGES", 2);
  static const int wgs = env_int("TTS_WARM_WGS", 120);
  static const int dist = env_int("TTS_WARM_XCD_DIST", 0);
  if (stages <= 0 || wgs < kWarmXcds) return WarmArgs{};
  const WgemmPlan pg = plan_wgemm(1, 2 * c.intermediate_size, c.hidden_size, EPI_SWIGLU, e->num_cu);
  // warm workgroup b is block first_block + b of its grid, `dist` XCDs before the gate/up block of that index
  return wgemm_warm_plan(pg, wgu, 2 * c.intermediate_size, c.hidden_size, stages, wgs, first_block - dist);
}
WgemmArgs Ctx::fused_attn_args(const AttnArgs& a, int layer, bool with_oproj) {
  WgemmArgs fx;
  fx.gran = w.gran.as<uint64_t>();
  fx.fa = a;
  fx.fattn_wgs = a.rows * a.KVH;
  fx.fattn_layer = layer;
  fx.fattn_err = w.ferr.as<int>() + FERR_GRANULE_TIMEOUT;
  // TTS_FATTN_SPINS: polls before a granule wait gives up (tests drive the failure path with it)
  static const int spins = std::max(1, env_int("TTS_FATTN_SPINS", 1 << 16));
  fx.fattn_spins = spins;
  if (with_oproj) {
    const LmLayer& ly = M.layers[layer];
    const WgemmPlan po = plan_wgemm(a.rows, c.hidden_size, c.num_heads * c.head_dim, EPI_RESID, e->num_cu);
    fx.fo_w = ly.wo;
    fx.fo_units = c.hidden_size / 16;
    fx.fo_ur = po.sp.ur();
    fx.fo_kc = po.sp.kc;
    fx.fo_resid = w.x.as<bf16_t>();
    if (a.rows == 1)  // (the fused launch runs the QKV plan's whole-unit grid, launch_wgemm)
      fx.warm = warm_args(ly.wgu, plan_wgemm(1, QKV(), c.hidden_size, EPI_STORE, e->num_cu).sp.grid + fx.fattn_wgs + fx.fo_units);
  }
  return fx;
}
// o_proj can ride the fused QKV + attention launch: its stream plan has the launch's shape
// (16 waves, 2-tile stages, K split 16 ways, one K chunk, two stages = the ring), one round
// of units, at most one unit per projection workgroup, 128 K values per wave
bool Ctx::fused_oproj_ok() const {
  if (!use_fused_oproj()) return false;
  const int HD = c.num_heads * c.head_dim, HID = c.hidden_size;
  const WgemmPlan pq = plan_wgemm(1, QKV(), HID, EPI_STORE, e->num_cu);
  const WgemmPlan po = plan_wgemm(1, HID, HD, EPI_RESID, e->num_cu);
  const StreamPlan& s = po.sp;
  return s.waves == 16 && s.ku == 2 && s.ksplit == 16 && s.kc == 1 && s.ng == 1 && HD == 16 * 128 &&
         (HD / 32) / (s.ksplit * s.ku) == 2 && HID / 16 <= s.ur() && HID / 16 <= pq.sp.grid &&
         pq.sp.waves == 16 && pq.sp.ku == 2 && pq.sp.ksplit == 16;
}

// 2..16 rows: o_proj can ride the fused QKV + attention launch when its stream plan has the
// launch's shape (16 waves, the QKV plan's stage width, K split 16 ways, the item = the
// two-stage ring) and o_proj's K is the hidden size (its A rows fit the launch's LDS rows)
bool Ctx::fused_oproj_rows_ok(int rows) const {
  if (!use_fused_oproj() || !use_fused_oproj_rows() || rows < 2 || rows > 16) return false;
  const int HD = c.num_heads * c.head_dim, HID = c.hidden_size;
  const WgemmPlan pq = plan_wgemm(rows, QKV(), HID, EPI_STORE, e->num_cu);
  const WgemmPlan po = plan_wgemm(rows, HID, HD, EPI_RESID, e->num_cu);
  const StreamPlan& s = po.sp;
  return HD == HID && s.waves == 16 && s.ksplit == 16 && s.ng == 1 && s.ku == pq.sp.ku && pq.sp.waves == 16 &&
         pq.sp.ksplit == 16 && (HD / 32) / (s.ksplit * s.ku) == 2 && (HD / 32) % (s.kc * s.ksplit * s.ku) == 0 &&
         HID / 16 <= s.ur() && (2 * s.ku) % 4 == 0;
}

void Ctx::layers(int rows, const int* slot, const int* pos, bool decode) {
  pending_norm = nullptr;  // w.x was rewritten (embeddings) since any earlier combine
  const bool fattn = fused_attn_ok(rows, decode);
  const bool foproj = fattn && (rows == 1 ? fused_oproj_ok() : fused_oproj_rows_ok(rows));
  // 17..32 decode rows: the attention may sum the QKV launch's partials (TTS_QKV_DEFER=0 keeps
  // the combine launch)
  const bool defer = decode && rows > 16 && rows <= 32 && use_qkv_defer();
  for (int l = 0; l < c.num_layers; ++l) {
    const LmLayer& ly = M.layers[l];
    // attention output (bf16 rows of w.attn_out): inside the QKV launch (one-row step), one
    // workgroup per (row, kv head) (decode), or per query block x kv head (prefill)
    if (fattn) {
      qkv_attn_proj(rows, ly, fused_attn_args(attn_args(l, rows, slot, pos), l, foproj));
    } else {
      const AttnArgs a = attn_args(l, rows, slot, pos, qkv_proj(rows, ly, defer));
      if (decode) {
        launch_attn_decode_step(a, s);
      } else {
        launch_rope_append(a, s);
        launch_attn_prefill(a, s);
      }
    }
    if (!foproj) {  // (decode: o_proj's combine may normalise with ln2 for the gate/up launch)
      if (decode || rows > kPrefillChunk) o_proj(rows, ly, ly.ln2);
      else o_proj(rows, ly);
    }
    gate_up(rows, ly);
    // (prefill GEMMs of > kPrefillChunk rows: the one-chunk form's combine may normalise too;
    // not after the last layer, whose rows only the gathered lm_head rows read)
    const bool last = l + 1 == c.num_layers;
    if (decode || (rows > kPrefillChunk && !last)) down_proj(rows, ly, last ? M.final_norm : M.layers[l + 1].ln1);
    else down_proj(rows, ly);
  }
}

StepState Ctx::state(int B, int eos, int min_new) {
  StepState st;
  auto ints = [&](int array) { return w.st_int.as<int>() + st_at(array, B, 0); };
  st.tokens = ints(ST_TOKENS); st.pos = ints(ST_POS); st.gen_count = ints(ST_GEN_COUNT); st.limit = ints(ST_LIMIT);
  st.done = ints(ST_DONE); st.eos_mask = ints(ST_EOS_MASK); st.n_active = ints(ST_N_ACTIVE);
  st.seen = w.seen.as<uint32_t>(); st.seen_stride = c.vocab_size / 32 + 1;
  st.counts = nullptr;  // (the caller's, when a frequency penalty is set)
  st.row_seed = w.row_seed.as<unsigned long long>();
  st.epoch = w.epoch.as<uint32_t>();
  st.out_ids = w.out_ids.as<int>(); st.out_stride = w.out_cap;
  st.eos_id = eos; st.min_new = min_new;
  st.par = nullptr;  // (the caller's, in a per-request slot batch)
  return st;
}

WgemmArgs Ctx::head_epilogue_args(const StepState& st, const tts_gen_params& gp) {
  WgemmArgs ex;
  ex.seen = st.seen; ex.seen_stride = st.seen_stride; ex.penalty = gp.repetition_penalty;
  ex.eos_mask = st.eos_mask;
  ex.part_val = w.lpart_v.as<float>(); ex.part_idx = w.lpart_i.as<int>(); ex.part_stride = LOGITS_MAX_PARTS;
  if (gp.do_sample) { ex.logits_out = w.slogits.as<float>(); ex.ldl = c.vocab_size; }
  ex.counts = st.counts; ex.freq_penalty = gp.frequency_penalty;
  return ex;
}

SampleArgs Ctx::sample_args(const StepState& st, const tts_gen_params& gp, bool lists, int nparts) {
  SampleArgs sa;
  sa.ldl = c.vocab_size; sa.V = c.vocab_size;
  sa.temperature = gp.temperature; sa.top_k = gp.top_k; sa.top_p = gp.top_p;
  sa.seed = gp.seed; sa.row_seed = st.row_seed; sa.step = st.gen_count; sa.done = st.done;
  sa.part_stride = LOGITS_MAX_PARTS;
  // the chosen token as the one "partial" finalize reads
  sa.out_part_val = w.lpart_v.as<float>(); sa.out_part_idx = w.lpart_i.as<int>();
  if (lists) {
    sa.logits = w.hcv.as<float>(); sa.list_idx = w.hci.as<int>(); sa.list_cnt = w.hcn.as<int>();
    sa.list_clear = 1; sa.vocab = c.vocab_size;
  } else {
    sa.logits = w.slogits.as<float>();
    sa.part_val = w.lpart_v.as<float>(); sa.nparts = nparts;
  }
  return sa;
}

// The argmax partials a full-head launch over B rows leaves per row: the tile head's column groups
// (the wide step), else the decode head's workgroups
int Ctx::head_parts(int B, int epi, bool step) const {
  if (step && B > kPrefillChunk && use_wide_head() && head_tile_supported(B, c.vocab_size, c.hidden_size))
    return head_tile_nparts(c.vocab_size);
  return plan_wgemm(std::min(B, kPrefillChunk), c.vocab_size, c.hidden_size, epi, e->num_cu).grid;
}

void Ctx::head_and_pick(const bf16_t* xin, int B, const StepState& st, const tts_gen_params& gp, bool step) {
  // greedy pick through the int8 screen + exact recheck (lm_head_screen.hip): the same ids as
  // the full lm_head launch below
  if (!gp.do_sample && M.head_grid && head_screen_supported(B, c.hidden_size, c.vocab_size)) {
    finalize(screened_head_parts(xin, B, st, gp), B, st);
    return;
  }
  // the sampled step through the screen: the int8 copy exists, the rows and top_k are covered
  // (every covered row count measured faster than the full head: DESIGN.md 3.6, no row gate)
  if (gp.do_sample && M.head_grid && head_screen_topk_supported(B, c.hidden_size, c.vocab_size, gp.top_k, M.head_grid)) {
    screened_sample(xin, B, st, gp);
    finalize(1, B, st);
    return;
  }
  TTS_REQUIRE(B <= kHeadTileMaxRows, "batch larger than the widest step");
  int nparts = head_parts(B, EPI_LOGITS, step);
  lm_head_pick(xin, B, head_epilogue_args(st, gp), EPI_LOGITS, step);
  if (gp.do_sample) {
    launch_sample(sample_args(st, gp, false, nparts), B, s);
    nparts = 1;
  }
  finalize(nparts, B, st);
}

// The per-request batch's pick: every row's settings from st.par (device memory), one kernel set
// for any mix of greedy and sampled rows.  Batches of 17..32 rows always take the full head: the
// screen's top-k mode covers 1..16 rows (8 at hidden 4096).
bool Ctx::rows_screen_ok(int B, int max_top_k) const {
  return M.head_grid && head_screen_topk_supported(B, c.hidden_size, c.vocab_size, std::max(1, max_top_k), M.head_grid);
}
void Ctx::head_and_pick_rows(const bf16_t* xin, int B, const StepState& st, bool dense, int max_top_k) {
  TTS_REQUIRE(st.par && st.counts, "per-row step without its settings table");
  tts_gen_params gp{};  // (neutral: the per-row kernels read none of it)
  gp.do_sample = 1; gp.repetition_penalty = 1.f; gp.temperature = 1.f; gp.top_k = 1; gp.top_p = 1.f;
  if (!dense && rows_screen_ok(B, max_top_k)) {
    screened_head_parts(xin, B, st, gp, std::max(1, max_top_k), st.par);
    SampleArgs sa = sample_args(st, gp, true);
    sample_rows_from_table(sa, st.par);
    launch_sample_list_rows(sa, B, s);
    finalize(1, B, st);
    return;
  }
  TTS_REQUIRE(B <= kHeadTileMaxRows, "batch larger than the widest step");
  const int nparts = head_parts(B, EPI_LOGITS_ROWS, true);  // (the per-row pick is the captured step's only)
  WgemmArgs ex = head_epilogue_args(st, gp);
  ex.row_par = st.par;
  lm_head_pick(xin, B, ex, EPI_LOGITS_ROWS, true);
  SampleArgs sa = sample_args(st, gp, false, nparts);
  sa.part_idx = w.lpart_i.as<int>();  // (a greedy row's argmax partials)
  sample_rows_from_table(sa, st.par);
  launch_sample_rows(sa, B, s);
  finalize(1, B, st);
}

// the sampled pick through the same screen (its top-k mode): the candidates of the top-k set,
// recomputed exactly, into per-row lists; the list sampler draws from them and leaves the token
// as the one "partial" finalize reads.  The ids of the full-head sampled step.
void Ctx::screened_sample(const bf16_t* xin, int B, const StepState& st, const tts_gen_params& gp) {
  screened_head_parts(xin, B, st, gp, gp.top_k);
  launch_sample_list(sample_args(st, gp, true), B, s);
}
// the screened head's launch (int8 screen + exact recompute of the units that can hold the
// argmax); returns the number of argmax partials per row.  top_k > 0: its top-k mode (the
// units that can hold a top-k candidate, into the candidate lists; no argmax partials)
int Ctx::screened_head_parts(const bf16_t* xin, int B, const StepState& st, const tts_gen_params& gp, int top_k,
                             const RowParams* par) {
  const int HID = c.hidden_size, V = c.vocab_size;
  HeadScreenArgs a;
  a.M = B; a.K = HID; a.ldx = HID; a.V = V;
  const bool ready = pending_norm == M.final_norm && xin == w.x.as<bf16_t>();  // (a residual combine
  if (ready) {                                                                 //  wrote RMSNorm(x, final norm))
    a.x = w.xn.as<bf16_t>();
  } else if (head_screen_prequant(B)) {
    launch_rmsnorm(xin, HID, M.final_norm, c.rms_norm_eps, w.xn.as<bf16_t>(), HID, B, HID, s);
    a.x = w.xn.as<bf16_t>();
  } else {
    a.x = xin; a.normw = M.final_norm; a.eps = c.rms_norm_eps;
  }
  if (head_screen_prequant(B)) {  // (17..32 rows: quantised once, not by every workgroup)
    launch_head_rowquant(a.x, HID, B, HID, w.hxq.as<int8_t>(), w.hxs.as<float>(), s);
    a.xq = w.hxq.as<int8_t>(); a.xstat = w.hxs.as<float>();
  }
  a.q = M.head_q.as<int8_t>(); a.cst = M.head_c.as<float4>();
  a.ur = M.head_grid * head_screen_waves();
  a.w = M.lm_head;
  const StreamPlan sp = stream_plan(V, HID, 1, e->num_cu);
  a.hku = sp.ku; a.hur = sp.ur(); a.hKT = HID / 32; a.hkc = sp.kc;
  a.seen = st.seen; a.seen_stride = st.seen_stride; a.penalty = gp.repetition_penalty;
  a.eos_mask = st.eos_mask; a.counts = st.counts; a.freq_penalty = gp.frequency_penalty;
  a.epoch = st.epoch; a.lbg = w.hlb.as<unsigned long long>();
  a.arrive = (uint32_t*)(w.hlb.as<unsigned long long>() + 32 * 8);
  a.spins = head_screen_wait(B, top_k > 0) ? (1 << 14) : 0;
  a.part_val = w.lpart_v.as<float>(); a.part_idx = w.lpart_i.as<int>(); a.part_stride = LOGITS_MAX_PARTS;
  if (head_screen_check()) {
    a.check = 1; a.ub = w.hub.as<float>(); a.ldu = V; a.err = w.ferr.as<int>() + FERR_SCREEN_CHECK;
  }
  if (top_k > 0) {
    a.top_k = top_k;
    a.slots = w.hslot.as<unsigned long long>();
    a.cand_val = w.hcv.as<float>(); a.cand_idx = w.hci.as<int>(); a.cand_cnt = w.hcn.as<int>(); a.ldc = V;
    if (a.check) a.lbo = w.hlo.as<float>();
    a.par = par;
  }
  static const int diag = env_int("TTS_HEAD_SCREEN_DIAG", 0);
  a.diag = diag;
  if (diag & 2) a.err = w.ferr.as<int>() + FERR_SCREEN_CHECK;  // (the count lands in FERR_SCREEN_DIAG)
  launch_head_screen(a, M.head_grid, s);
  return M.head_grid;
}

std::vector<int> Ctx::prefill_group(const int32_t* ids, const int32_t* lens, int nb, int slot_base, int gather_row) {
  std::vector<int> slot, pos, tok, blk, last_rows(nb);
  int rows = 0;
  for (int b = 0; b < nb; ++b) {
    for (int i = 0; i < lens[b]; ++i) tok.push_back(ids[rows + i]);
    // query rows and attention query blocks (up to 16 consecutive rows of one sequence)
    prefill_seq_rows(slot_base + b, 0, lens[b], rows, slot, pos, blk);
    rows += lens[b];
    last_rows[b] = rows - 1;
  }
  TTS_REQUIRE(rows <= w.cap_rows, "total prompt rows exceed the prefill workspace");
  w.nblocks = (int)blk.size() / 4;
  HIP_CHECK(hipMemcpyAsync(w.blocks.p, blk.data(), blk.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(w.row_slot.p, slot.data(), rows * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(w.row_pos.p, pos.data(), rows * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(w.row_idx.p, tok.data(), rows * 4, hipMemcpyHostToDevice, s));
  launch_embed(w.row_idx.as<int>(), M.embed_rows.as<bf16_t>(), w.x.as<bf16_t>(), rows, c.hidden_size, s);
  // the fused QKV + attention launch tags its granules (position, layer): a sequence starting
  // over at a position an earlier sequence reached must not find that sequence's granules
  // (with a matching tag the attention workgroups could read them before this step's QKV
  // workgroups overwrite them)
  HIP_CHECK(hipMemsetAsync(w.gran.p, 0xff, w.gran.bytes, s));
  layers(rows, w.row_slot.as<int>(), w.row_pos.as<int>(), false);
  if (gather_row >= 0) {
    HIP_CHECK(hipMemcpyAsync(w.row_idx.p, last_rows.data(), nb * 4, hipMemcpyHostToDevice, s));
    launch_gather_rows(w.x.as<bf16_t>(), c.hidden_size, w.row_idx.as<int>(),
                       w.last_x.as<bf16_t>() + (size_t)gather_row * c.hidden_size, nb, c.hidden_size, s);
  }
  return last_rows;
}

void Ctx::prefill_all(const int32_t* ids, const std::vector<int>& start, const std::vector<int>& lens,
                      bool gather_last, const char* what) {
  const int B = (int)lens.size();
  for (int b0 = 0, b1 = 0; b0 < B; b0 = b1) {
    int grp = 0;
    std::vector<int32_t> gid;
    while (b1 < B && grp + lens[b1] <= w.cap_rows) {
      gid.insert(gid.end(), ids + start[b1], ids + start[b1] + lens[b1]);
      grp += lens[b1++];
    }
    TTS_REQUIRE(b1 > b0, std::string("a ") + what + " is longer than the prefill workspace");
    prefill_group(gid.data(), lens.data() + b0, b1 - b0, b0, gather_last ? b0 : -1);
  }
}

// The launch list of one decode step over `rows` rows of a model of config c on num_cu CUs,
// without a GPU: the step's own code (Ctx::layers + head_and_pick) run with the launchers in
// dry-run mode (lm_kernels.h dry_launches), nothing allocated.  Unique launches in first-seen
// order, one per line (wgemm instantiations as wgemm_inst_name writes them).
std::string lm_step_plan(const tts_lm_config& c, int rows, int num_cu, int top_k, bool per_row) {
  TTS_REQUIRE(c.head_dim == 64 || c.head_dim == 128, "head_dim must be 64 or 128");
  TTS_REQUIRE(c.num_heads == 4 * c.num_kv_heads && c.num_layers >= 1, "bad config");
  TTS_REQUIRE(rows >= 1 && rows <= kHeadTileMaxRows && num_cu >= 1, "rows in [1, 256], num_cu >= 1");
  Engine e;  // (no HIP call: no stream, no buffer)
  e.num_cu = num_cu;
  e.lm.cfg = c;
  e.lm.cfg.max_batch = std::max(c.max_batch, rows);
  // distinct placeholder addresses for the weights (the step code compares norm-weight pointers
  // to choose its RMSNorm form; nothing is dereferenced in a dry run)
  uintptr_t fake = 0x10000;
  auto next = [&] { fake += 0x100; return (bf16_t*)fake; };
  e.lm.layers.resize(c.num_layers);
  for (LmLayer& ly : e.lm.layers) {
    ly.ln1 = next(); ly.ln2 = next(); ly.wqkv = next(); ly.wo = next(); ly.wgu = next(); ly.wd = next();
  }
  e.lm.final_norm = next();
  e.lm.lm_head = next();
  e.lm.head_grid = head_screen_grid(c, num_cu);
  e.w.cap_batch = e.lm.cfg.max_batch;
  e.w.kpart.bytes = kpart_bytes(c);  // (the sizes the plan checks; never dereferenced)
  e.w.ppart.bytes = ppart_bytes(c);
  std::vector<std::string> rec;
  dry_launches() = &rec;
  try {
    Ctx X(&e, nullptr);
    X.layers(rows, nullptr, nullptr, true);
    StepState st = X.state(rows, 0, 0);
    tts_gen_params gp{};
    gp.repetition_penalty = 1.1f;
    if (top_k > 0) {  // a sampled step
      gp.do_sample = 1; gp.temperature = 0.8f; gp.top_k = top_k; gp.top_p = 1.0f;
    }
    if (per_row) {  // (placeholder addresses, as the weights': never dereferenced)
      st.par = (const RowParams*)next();
      st.counts = (uint16_t*)next();
      X.head_and_pick_rows(nullptr, rows, st, !X.rows_screen_ok(rows, top_k), top_k);
    } else {
      X.head_and_pick(nullptr, rows, st, gp, true);
    }
  } catch (...) {
    dry_launches() = nullptr;
    e.w.kpart.bytes = 0;
    e.w.ppart.bytes = 0;
    throw;
  }
  dry_launches() = nullptr;
  e.w.kpart.bytes = 0;
  e.w.ppart.bytes = 0;
  std::string out;
  std::vector<std::string> seen;
  for (const std::string& r : rec)
    if (std::find(seen.begin(), seen.end(), r) == seen.end()) {
      seen.push_back(r);
      out += r + "\n";
    }
  return out;
}

}  // namespace tts
