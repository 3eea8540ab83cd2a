// lm_generate.cpp — SpeechLM generation: prefill, the hipGraph-captured decode step, the
// generate loop with device-side stop bookkeeping, and continuous-batching slots.
//
// Replaces the reference AR loop `_generate_speech_tokens` -> HF `model.generate`
// (tts/inference/inferencing.py:94-107; transformers generation/utils.py:2783-2950):
//   * prefill over the prompt, then one decode step per generated code;
//   * greedy: argmax over fp32(bf16 logits) after repetition penalty and min-new-tokens EOS
//     mask; stop at EOS (included in the output) or at max_length (total length);
//   * batch > 1 = independent sequences (each identical to its batch-1 generate).
// HF syncs the host every token (`unfinished_sequences.max() == 0`); here the step is one
// hipGraph replay and the host polls a device counter of active sequences every
// kPollEvery steps, one poll behind, so the GPU never waits for the host.
#include "lm_step.h"

namespace tts {

static constexpr int kPollEvery = 8;

// The decode step (all layers + lm_head + pick + finalize over B rows) captured once into a
// hipGraph, recaptured when what it bakes in (StepKey) changes.
// per_row: the per-request batch's step (settings in LmWork::row_par; max_top_k / dense choose its form)
static void ensure_step_graph(Engine* e, int B, const StepState& st, const tts_gen_params& gp, bool per_row = false,
                              bool dense = false, int max_top_k = 1) {
  LmWork& W = e->w;
  const StepKey key = per_row ? StepKey::rows(B, dense) : StepKey(B, gp);
  if (W.graph && !(W.step_key == key)) {
    (void)hipGraphExecDestroy(W.graph);
    W.graph = nullptr;
  }
  if (W.graph) return;
  hipStream_t cs;
  HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipGraph_t g;
  HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  Ctx Y(e, cs);
  Y.layers(B, W.row_slot.as<int>(), st.pos, true);
  if (per_row) Y.head_and_pick_rows(W.x.as<bf16_t>(), B, st, dense, max_top_k);
  else Y.head_and_pick(W.x.as<bf16_t>(), B, st, gp, true);
  HIP_CHECK(hipStreamEndCapture(cs, &g));
  HIP_CHECK(hipGraphInstantiate(&W.graph, g, nullptr, nullptr, 0));
  HIP_CHECK(hipGraphDestroy(g));
  HIP_CHECK(hipStreamDestroy(cs));
  W.step_key = key;
}

// the sampling parameters a generation or a slot batch runs with
static void validate_gen_params(const tts_gen_params* p) {
  TTS_REQUIRE(p != nullptr, "null argument");
  if (p->do_sample) {  // HF: TemperatureLogitsWarper requires T > 0; top_k from GenerationConfig (50)
    TTS_REQUIRE(p->temperature > 0.f, "sampling needs temperature > 0 (temperature 0 = greedy)");
    TTS_REQUIRE(p->top_k >= 1 && p->top_k <= SAMPLE_MAX_TOP_K,
                "sampling supports top_k in [1, 1024] (HF default 50; full-vocabulary sampling is not built)");
    TTS_REQUIRE(p->top_p > 0.f && p->top_p <= 1.f, "top_p must be in (0, 1]");
  }
  TTS_REQUIRE(std::isfinite(p->frequency_penalty), "frequency_penalty must be finite");
}
// ... of a per-request batch (its defaults and every request's own): the penalty divides every
// row's seen logits, idle rows included
static void validate_row_params(const tts_gen_params* p) {
  validate_gen_params(p);
  TTS_REQUIRE(std::isfinite(p->repetition_penalty) && p->repetition_penalty > 0.f,
              "repetition_penalty must be finite and > 0");
  TTS_REQUIRE(std::isfinite(p->temperature) && p->temperature >= 0.f, "temperature must be finite and >= 0");
}
// a request's row of the settings table (a greedy row: top_k 1, the screen's k)
static RowParams row_params(const tts_gen_params& p) {
  RowParams r;
  r.penalty = p.repetition_penalty; r.freq_penalty = p.frequency_penalty;
  r.temperature = p.do_sample ? p.temperature : 1.f; r.top_p = p.do_sample ? p.top_p : 1.f;
  r.top_k = p.do_sample ? p.top_k : 1; r.eos_id = p.eos_token_id; r.min_new = p.min_new_tokens;
  r.sample = p.do_sample ? 1 : 0;
  return r;
}

void lm_gen_begin(Engine* e, const tts_gen_params* p, const int32_t* ids, const int32_t* lens, int B,
                  hipStream_t s) {
  TTS_REQUIRE(e->lm.loaded, "tts_lm_load has not been called");
  e->slots.open = false;
  TTS_REQUIRE(p != nullptr && ids != nullptr && lens != nullptr, "null argument");
  TTS_REQUIRE(B >= 1 && B <= e->w.cap_batch, "batch out of range");
  validate_gen_params(p);
  Ctx X(e, s);
  const tts_lm_config& c = X.c;
  const int V = c.vocab_size;
  // ---- host-side state init
  std::vector<int> st_host = st_zeros(B), start(B), plen(lens, lens + B);
  std::vector<uint32_t> seen((size_t)B * (V / 32 + 1), 0u);
  int max_new = 0, off = 0;
  for (int b = 0; b < B; ++b) {
    const int P = lens[b];
    TTS_REQUIRE(P >= 1, "empty prompt");
    // HF: max_length counts the prompt; input length >= max_length is a ValueError
    // (generation/utils.py _validate_generated_length)
    TTS_REQUIRE(P < p->max_length, "input length >= max_length");
    const int limit = p->max_length - P;
    TTS_REQUIRE(P + limit <= c.max_seq_len, "prompt + max new tokens exceed max_seq_len");
    TTS_REQUIRE(limit <= e->w.out_cap, "max new tokens exceed the output capacity");
    for (int i = 0; i < P; ++i) {
      const int t = ids[off + i];
      TTS_REQUIRE(t >= 0 && t < V, "token id out of range");
      seen[(size_t)b * (V / 32 + 1) + (t >> 5)] |= 1u << (t & 31);
    }
    start[b] = off;
    off += P;
    st_host[st_at(ST_POS, B, b)] = P - 1;  // finalize advances it to P for the first new token
    st_host[st_at(ST_LIMIT, B, b)] = limit;
    st_host[st_at(ST_EOS_MASK, B, b)] = (p->min_new_tokens > 0) ? p->eos_token_id : -1;
    max_new = std::max(max_new, limit);
  }
  st_host[st_at(ST_N_ACTIVE, B, 0)] = B;
  StepState st = X.state(B, p->eos_token_id, p->min_new_tokens);
  if (p->frequency_penalty != 0.f) {  // vLLM form: counts of the new tokens only
    st.counts = e->w.counts.as<uint16_t>();
    HIP_CHECK(hipMemsetAsync(st.counts, 0, (size_t)B * st.seen_stride * 32 * 2, s));
  }
  HIP_CHECK(hipMemcpyAsync(e->w.st_int.p, st_host.data(), st_host.size() * 4,
                           hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(e->w.seen.p, seen.data(), seen.size() * 4, hipMemcpyHostToDevice, s));
  {  // row b draws with key seed + GOLD * (b << 32)  (rng_uniform(key, 0, step))
    std::vector<unsigned long long> rs(B);
    for (int b = 0; b < B; ++b) rs[b] = p->seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)b << 32);
    HIP_CHECK(hipMemcpyAsync(e->w.row_seed.p, rs.data(), B * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (rs is a stack buffer)
  }
  HIP_CHECK(hipEventRecord(e->ev[2], s));

  // ---- prefill, then the first token from every prompt's last row
  X.prefill_all(ids, start, plen, true, "prompt");
  X.head_and_pick(e->w.last_x.as<bf16_t>(), B, st, *p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(e->ev[3], s));

  // ---- decode: identity slot map; positions live in the step state
  X.upload_identity_slots(B);
  // (the embedding of each sequence's next token is already in w.x rows 0..B-1)
  ensure_step_graph(e, B, st, *p);
  Engine::Gen& G = e->gen;
  G.open = true;
  G.B = B;
  G.max_new = max_new;
  G.launched = 1;  // the prefill's head produced the first token
  G.polls = 0;
  G.finished = max_new <= 1;
  G.s = s;
  e->decode_steps = 0;
}

static int read_int(const int* dev, hipStream_t s) {  // (synchronises the stream)
  int v = 0;
  HIP_CHECK(hipMemcpyAsync(&v, dev, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return v;
}

// Up to n_steps decode-step graph replays.  The host polls the device's active-row counter
// every kPollEvery steps, one poll behind (no per-step D->H sync; HF syncs every step,
// generation/utils.py:2936-2937): a stopped row runs idle (its kernels skip it) until the
// poll sees every row done.
int lm_gen_continue(Engine* e, int n_steps) {
  Engine::Gen& G = e->gen;
  TTS_REQUIRE(G.open, "no generation in progress (tts_generate_begin)");
  const hipStream_t s = G.s;
  const StepState st = Ctx(e, s).state(G.B, e->w.step_key.eos, e->w.step_key.min_new);
  for (int n = 0; n < n_steps && !G.finished; ++n) {
    if (G.launched >= G.max_new) { G.finished = true; break; }
    HIP_CHECK(hipGraphLaunch(e->w.graph, s));
    ++G.launched;
    ++e->decode_steps;
    if (G.launched % kPollEvery == 0) {
      const int slot = G.polls & 1;
      HIP_CHECK(hipMemcpyAsync(&e->w.h_active[slot], st.n_active, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipEventRecord(e->ev[slot], s));
      if (G.polls > 0) {
        HIP_CHECK(hipEventSynchronize(e->ev[slot ^ 1]));
        if (e->w.h_active[slot ^ 1] == 0) G.finished = true;
      }
      ++G.polls;
    }
  }
  if (G.launched >= G.max_new) G.finished = true;
  // exact answer for a streaming caller: sync once per chunk
  if (!G.finished && read_int(st.n_active, s) == 0) G.finished = true;
  return G.finished ? 1 : 0;
}

// What the step's kernels flagged since the last read (LmWork::ferr), cleared for the next
// generation.  A fused QKV+attention launch whose granule wait timed out leaves garbage, and a
// check-mode screened head may find a score outside its bound: fail loudly at this read.
void read_device_flags(Engine* e, hipStream_t s) {
  if (!e->w.ferr.p) return;
  int* ferr = e->w.ferr.as<int>();
  int err[FERR_SLOTS] = {};
  HIP_CHECK(hipMemcpyAsync(err, ferr, sizeof(err), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (err[FERR_SCREEN_DIAG]) {  // (TTS_HEAD_SCREEN_DIAG=2: units the screen recomputed since the last read)
    fprintf(stderr, "head screen: %d units recomputed\n", err[FERR_SCREEN_DIAG]);
    HIP_CHECK(hipMemsetAsync(ferr + FERR_SCREEN_DIAG, 0, 4, s));
  }
  if (err[FERR_GRANULE_TIMEOUT] || err[FERR_SCREEN_CHECK]) {
    HIP_CHECK(hipMemsetAsync(ferr, 0, 8, s));  // (the two error flags: slots 0 and 1)
    HIP_CHECK(hipStreamSynchronize(s));
    TTS_REQUIRE(!err[FERR_GRANULE_TIMEOUT], "fused QKV+attention: a granule wait timed out (results invalid)");
    TTS_REQUIRE(false, "screened lm_head: an exact score outside its int8 bound (TTS_HEAD_SCREEN_CHECK)");
  }
}

void lm_gen_read(Engine* e, int32_t* out_ids, int out_stride, int32_t* out_lens) {
  Engine::Gen& G = e->gen;
  TTS_REQUIRE(G.open, "no generation in progress (tts_generate_begin)");
  const hipStream_t s = G.s;
  const StepState st = Ctx(e, s).state(G.B, e->w.step_key.eos, e->w.step_key.min_new);
  std::vector<int> gc(G.B);
  HIP_CHECK(hipMemcpyAsync(gc.data(), st.gen_count, G.B * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  read_device_flags(e, s);
  for (int b = 0; b < G.B; ++b) {
    TTS_REQUIRE(gc[b] <= out_stride, "out_stride too small");
    out_lens[b] = gc[b];
    HIP_CHECK(hipMemcpy(out_ids + (size_t)b * out_stride, st.out_ids + (size_t)b * st.out_stride,
                        (size_t)gc[b] * 4, hipMemcpyDeviceToHost));
  }
}

void lm_generate(Engine* e, const tts_gen_params* p, const int32_t* ids, const int32_t* lens,
                 int B, int32_t* out_ids, int out_stride, int32_t* out_lens, hipStream_t s) {
  for (int b = 0; b < B; ++b)
    TTS_REQUIRE(p->max_length - lens[b] <= out_stride, "out_stride too small");
  lm_gen_begin(e, p, ids, lens, B, s);
  const int max_new = e->gen.max_new;
  lm_gen_continue(e, max_new);
  HIP_CHECK(hipEventRecord(e->ev[1], s));
  lm_gen_read(e, out_ids, out_stride, out_lens);
  float t0 = 0.f, t1 = 0.f;
  HIP_CHECK(hipEventElapsedTime(&t0, e->ev[2], e->ev[3]));
  HIP_CHECK(hipEventElapsedTime(&t1, e->ev[3], e->ev[1]));
  e->t_prefill_ms = t0;
  e->t_decode_ms = t1;
  e->gen.open = false;
}

// ---------------------------------------------------------------- continuous batching --
// S persistent rows (slots) share one captured decode step; a sequence is admitted into a
// free slot between chunks (its prompt prefilled into that slot's KV strip, its first token
// picked, its step-state row initialised) and retired when it stops.  Rows never mix, so
// every sequence's tokens equal a batch-1 generate of its prompt with the shared settings.
static StepState slots_state(Engine* e, hipStream_t s) {
  Engine::Slots& Z = e->slots;
  StepState st = Ctx(e, s).state(Z.S, Z.gp.eos_token_id, Z.gp.min_new_tokens);
  if (Z.gp.frequency_penalty != 0.f || Z.per_row) st.counts = e->w.counts.as<uint16_t>();
  if (Z.per_row) st.par = e->w.row_par.as<RowParams>();
  return st;
}

void lm_slots_open(Engine* e, const tts_gen_params* p, int S, hipStream_t s, bool per_request) {
  TTS_REQUIRE(e->lm.loaded, "tts_lm_load has not been called");
  if (per_request) validate_row_params(p);
  else validate_gen_params(p);
  TTS_REQUIRE(S >= 1 && S <= e->w.cap_batch, "slot count out of range (max_batch)");
  e->gen.open = false;
  Engine::Slots& Z = e->slots;
  Z.open = true;
  Z.S = S;
  Z.gp = *p;
  Z.busy.assign(S, 0);
  Z.next_req = 0;
  Z.s = s;
  Z.per_row = per_request;
  Z.max_top_k = p->do_sample ? p->top_k : 1;
  const int V = e->lm.cfg.vocab_size;
  // (above the screen's top_k bound from the start: the full head)
  Z.dense = per_request && !Ctx(e, s).rows_screen_ok(S, Z.max_top_k);
  if (per_request) {  // every row holds valid settings (idle rows are computed too): the defaults
    const std::vector<RowParams> tab((size_t)S, row_params(*p));
    HIP_CHECK(hipMemcpyAsync(e->w.row_par.p, tab.data(), tab.size() * sizeof(RowParams), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(e->w.counts.p, 0, (size_t)S * (V / 32 + 1) * 32 * 2, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (tab is a local buffer)
  }
  // every row idle: done = 1, n_active = 0, no EOS mask
  std::vector<int> st_host = st_zeros(S);
  for (int b = 0; b < S; ++b) { st_host[st_at(ST_DONE, S, b)] = 1; st_host[st_at(ST_EOS_MASK, S, b)] = -1; }
  HIP_CHECK(hipMemcpyAsync(e->w.st_int.p, st_host.data(), st_host.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(e->w.seen.p, 0, (size_t)S * (V / 32 + 1) * 4, s));
  Ctx(e, s).upload_identity_slots(S);
  const StepState st = slots_state(e, s);
  ensure_step_graph(e, S, st, Z.gp, Z.per_row, Z.dense, Z.max_top_k);
  HIP_CHECK(hipStreamSynchronize(s));
}

// seed: the request's sampling key (vLLM SamplingParams.seed); nullptr = the batch seed
// mixed with a request counter, so every request draws its own stream
void lm_slots_add(Engine* e, int slot, const int32_t* prompt, int len, int max_new, const uint64_t* seed,
                  const tts_gen_params* rp) {
  Engine::Slots& Z = e->slots;
  TTS_REQUIRE(Z.open, "no slot batch open (tts_slots_open)");
  if (rp && !Z.per_row) throw Error(TTS_E_STATE, "per-request settings need tts_slots_open_per_request");
  if (rp) validate_row_params(rp);  // (before anything is written: a bad request leaves every row as it was)
  tts_gen_params gp = rp ? *rp : Z.gp;  // the request's settings (seed and max_length: the batch's)
  gp.seed = Z.gp.seed; gp.max_length = Z.gp.max_length;
  TTS_REQUIRE(slot >= 0 && slot < Z.S && !Z.busy[slot], "slot out of range or busy");
  TTS_REQUIRE(prompt != nullptr && len >= 1, "empty prompt");
  const tts_lm_config& c = e->lm.cfg;
  const int V = c.vocab_size;
  TTS_REQUIRE(max_new >= 1 && len + max_new <= c.max_seq_len && max_new <= e->w.out_cap,
              "prompt + max new tokens exceed max_seq_len");
  TTS_REQUIRE(len <= e->w.cap_rows, "prompt longer than the prefill workspace");
  const hipStream_t s = Z.s;
  Ctx X(e, s);
  StepState st = slots_state(e, s);
  const int S = Z.S, stride = st.seen_stride;
  // ---- the slot's step-state row (and its penalty set) on the device
  std::vector<uint32_t> seen((size_t)stride, 0u);
  for (int i = 0; i < len; ++i) {
    TTS_REQUIRE(prompt[i] >= 0 && prompt[i] < V, "token id out of range");
    seen[prompt[i] >> 5] |= 1u << (prompt[i] & 31);
  }
  HIP_CHECK(hipMemcpyAsync(st.seen + (size_t)slot * stride, seen.data(), (size_t)stride * 4,
                           hipMemcpyHostToDevice, s));
  if (st.counts) HIP_CHECK(hipMemsetAsync(st.counts + (size_t)slot * stride * 32, 0, (size_t)stride * 32 * 2, s));
  int row[ST_N_ACTIVE] = {};  // (tokens, gen_count and done start at 0)
  row[ST_POS] = len - 1;
  row[ST_LIMIT] = max_new;
  row[ST_EOS_MASK] = (gp.min_new_tokens > 0) ? gp.eos_token_id : -1;
  for (int k = 0; k < ST_N_ACTIVE; ++k)
    HIP_CHECK(hipMemcpyAsync(e->w.st_int.as<int>() + st_at(k, S, slot), &row[k], 4, hipMemcpyHostToDevice, s));
  // the row's sampling key: the same for its first token (drawn below as a batch of 1) and
  // for every decode step (row = slot)
  const unsigned long long key =
      seed ? (unsigned long long)*seed : Z.gp.seed + 0x9E3779B97F4A7C15ull * ((++Z.next_req) << 32);
  HIP_CHECK(hipMemcpyAsync(st.row_seed + slot, &key, 8, hipMemcpyHostToDevice, s));
  const int act = read_int(st.n_active, s) + 1;
  HIP_CHECK(hipMemcpyAsync(st.n_active, &act, 4, hipMemcpyHostToDevice, s));
  // ---- prefill the prompt into the slot's KV strip, pick its first token
  X.prefill_group(prompt, &len, 1, slot, 0);
  if (Z.per_row) {
    // the row's settings for the captured step; a request above the screen's top_k bound moves the
    // step to the full head (one recapture; stays until the batch is reopened)
    const RowParams r = row_params(gp);
    HIP_CHECK(hipMemcpyAsync(e->w.row_par.as<RowParams>() + slot, &r, sizeof r, hipMemcpyHostToDevice, s));
    Z.max_top_k = std::max(Z.max_top_k, r.top_k);
    if (!Z.dense && !X.rows_screen_ok(S, Z.max_top_k)) Z.dense = true;
    HIP_CHECK(hipStreamSynchronize(s));  // (r is a stack buffer)
  }
  // the first token: the uniform kernels over a batch of 1, given the request's settings
  StepState one = step_state_row(st, slot);
  one.par = nullptr;
  one.eos_id = gp.eos_token_id; one.min_new = gp.min_new_tokens;
  if (Z.per_row && gp.frequency_penalty == 0.f) one.counts = nullptr;  // (as a uniform batch without the penalty)
  X.head_and_pick(e->w.last_x.as<bf16_t>(), 1, one, gp);
  // the prefill overwrote the decode rows of w.x: re-embed every row's next token
  X.upload_identity_slots(S);
  launch_embed(st.tokens, e->lm.embed_rows.as<bf16_t>(), e->w.x.as<bf16_t>(), S, c.hidden_size, s);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  if (Z.per_row) ensure_step_graph(e, S, st, Z.gp, true, Z.dense, Z.max_top_k);  // (recaptured when dense flipped)
  Z.busy[slot] = 1;
}

int lm_slots_step(Engine* e, int n_steps) {
  Engine::Slots& Z = e->slots;
  TTS_REQUIRE(Z.open, "no slot batch open (tts_slots_open)");
  const StepState st = slots_state(e, Z.s);
  for (int n = 0; n < n_steps; ++n) HIP_CHECK(hipGraphLaunch(e->w.graph, Z.s));
  read_device_flags(e, Z.s);
  return read_int(st.n_active, Z.s);
}

void lm_slots_read(Engine* e, int slot, int32_t* out_ids, int cap, int32_t* n_out, int32_t* finished) {
  Engine::Slots& Z = e->slots;
  TTS_REQUIRE(Z.open, "no slot batch open (tts_slots_open)");
  TTS_REQUIRE(slot >= 0 && slot < Z.S, "slot out of range");
  const StepState st = slots_state(e, Z.s);
  int gc = 0, dn = 0;
  HIP_CHECK(hipMemcpyAsync(&gc, st.gen_count + slot, 4, hipMemcpyDeviceToHost, Z.s));
  HIP_CHECK(hipMemcpyAsync(&dn, st.done + slot, 4, hipMemcpyDeviceToHost, Z.s));
  HIP_CHECK(hipStreamSynchronize(Z.s));
  TTS_REQUIRE(gc <= cap, "output capacity too small");
  if (gc > 0)
    HIP_CHECK(hipMemcpy(out_ids, st.out_ids + (size_t)slot * st.out_stride, (size_t)gc * 4, hipMemcpyDeviceToHost));
  *n_out = gc;
  *finished = Z.busy[slot] ? dn : 1;
}

void lm_slots_release(Engine* e, int slot) {
  Engine::Slots& Z = e->slots;
  TTS_REQUIRE(Z.open, "no slot batch open (tts_slots_open)");
  TTS_REQUIRE(slot >= 0 && slot < Z.S, "slot out of range");
  if (!Z.busy[slot]) return;
  const StepState st = slots_state(e, Z.s);
  if (!read_int(st.done + slot, Z.s)) {  // aborted while running: stop the row and drop it from the active count
    int act = 0;
    const int one = 1;
    HIP_CHECK(hipMemcpy(st.done + slot, &one, 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(&act, st.n_active, 4, hipMemcpyDeviceToHost));
    --act;
    HIP_CHECK(hipMemcpy(st.n_active, &act, 4, hipMemcpyHostToDevice));
  }
  Z.busy[slot] = 0;
}

}  // namespace tts
