// lm_debug.cpp — entry points that measure or inspect the SpeechLM step rather than generate with
// it: the per-kernel bench selectors, teacher-forced scoring through the prefill and through the
// decode kernels, and the diagnostic build's stamps buffer.
#include "lm_step.h"

namespace tts {

#ifdef TTS_STAMPS
// diagnostic build only: per-workgroup clock stamps of the last launches (scripts/stamp_probe.py)
static unsigned long long* g_stamps = nullptr;
constexpr int kStampSlots = 1 << 16;
unsigned long long* stamp_buf() {
  if (!g_stamps) {
    HIP_CHECK(hipMalloc((void**)&g_stamps, kStampSlots * 8));
    HIP_CHECK(hipMemset(g_stamps, 0, kStampSlots * 8));
  }
  return g_stamps;
}
extern "C" int tts_debug_stamps(unsigned long long* host, int n) {
  if (!g_stamps || n > kStampSlots) return 1;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpy(host, g_stamps, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return hipMemset(g_stamps, 0, kStampSlots * 8) == hipSuccess ? 0 : 1;
}
#else
unsigned long long* stamp_buf() { return nullptr; }
#endif

void lm_bench_kernel(Engine* e, int which, int rows, int ctx, int iters, float* avg_ms,
                     double* bytes) {
  TTS_REQUIRE(e->lm.loaded, "tts_lm_load has not been called");
  TTS_REQUIRE(rows >= 1 && rows <= e->w.cap_batch, "rows out of range");
  TTS_REQUIRE(ctx >= 1 && ctx <= e->lm.cfg.max_seq_len, "ctx out of range");
  TTS_REQUIRE(which >= 0 && which <= 12 && iters >= 1, "bad kernel selector");
  hipStream_t s = e->stream;
  Ctx X(e, s);
  const tts_lm_config& c = X.c;
  const int HID = c.hidden_size, HD = c.num_heads * c.head_dim, FF = c.intermediate_size;
  const int V = c.vocab_size, QKV = X.QKV(), hgrid = X.M.head_grid;
  TTS_REQUIRE(which < 6 || which > 7 || X.fused_attn_ok(rows, true), "fused QKV+attention does not apply to this shape");
  TTS_REQUIRE(which != 10 || (hgrid && head_screen_topk_supported(rows, HID, V, 50, hgrid)),
              "the screened sampling head does not apply to this shape (or is off)");
  TTS_REQUIRE(which < 8 || which > 9 || (hgrid && rows <= 32 && head_screen_supported(rows, HID, V)),
              "the screened lm_head does not apply to this shape (or is off)");
  TTS_REQUIRE(which != 7 || (rows == 1 ? X.fused_oproj_ok() : X.fused_oproj_rows_ok(rows)),
              "fused o_proj does not apply to this shape (or is off)");
  std::vector<int> tok(rows), pos(rows, ctx - 1);
  for (int r = 0; r < rows; ++r) tok[r] = (r * 7919 + 11) % V;
  HIP_CHECK(hipMemcpyAsync(e->w.row_idx.p, tok.data(), rows * 4, hipMemcpyHostToDevice, s));
  X.upload_identity_slots(rows);
  HIP_CHECK(hipMemcpyAsync(e->w.row_pos.p, pos.data(), rows * 4, hipMemcpyHostToDevice, s));
  launch_embed(e->w.row_idx.as<int>(), X.M.embed_rows.as<bf16_t>(), e->w.x.as<bf16_t>(), rows, HID, s);
  const LmLayer& ly = X.M.layers[0];
  StepState st = X.state(rows, -1, 0);
  std::vector<int> zeros = st_zeros(rows);
  for (int r = 0; r < rows; ++r) zeros[st_at(ST_EOS_MASK, rows, r)] = -1;  // no EOS mask
  HIP_CHECK(hipMemcpyAsync(e->w.st_int.p, zeros.data(), zeros.size() * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(e->w.seen.p, 0, (size_t)rows * st.seen_stride * 4, s));
  // real activations for every stage
  X.qkv_proj(rows, ly);
  HIP_CHECK(hipMemsetAsync(e->w.attn_out.p, 0, (size_t)rows * HD * 2, s));
  HIP_CHECK(hipMemsetAsync(e->w.act.p, 0, (size_t)rows * FF * 2, s));
  AttnArgs aa = X.attn_args(0, rows, e->w.row_slot.as<int>(), e->w.row_pos.as<int>());
  tts_gen_params greedy{}, sampled{};  // the heads' settings
  greedy.repetition_penalty = sampled.repetition_penalty = 1.1f;
  sampled.do_sample = 1; sampled.temperature = 0.8f; sampled.top_k = 50; sampled.top_p = 1.0f;
  const WgemmArgs ex = X.head_epilogue_args(st, greedy), sx = X.head_epilogue_args(st, sampled);
  launch_attn_decode_step(aa, s);  // (a real attention row for o_proj)
  double b = 0;
  const double act_rw = 2.0 * rows;
  // launches rotate over the layers (as the decode step does), so a layer's weights are
  // not still cached from the previous launch: the timing reflects HBM streaming
  int it_layer = 0;
  auto launch = [&]() {
    const int li = it_layer++ % c.num_layers;
    const LmLayer& ly = X.M.layers[li];
    switch (which) {
      case 0:
        X.qkv_proj(rows, ly);
        b = 2.0 * QKV * HID + act_rw * (HID + QKV) + 2.0 * HID;
        break;
      case 1:  // (1 and 3: without the next norm the step's combine carries at 10..32 rows)
        X.o_proj(rows, ly);
        b = 2.0 * HID * HD + act_rw * (HD + 2 * HID);
        break;
      case 2:
        X.gate_up(rows, ly);
        b = 2.0 * 2 * FF * HID + act_rw * (HID + FF) + 2.0 * HID;
        break;
      case 3:
        X.down_proj(rows, ly);
        b = 2.0 * HID * FF + act_rw * (FF + 2 * HID);
        break;
      case 4:
        X.pending_norm = nullptr;
        X.lm_head_pick(e->w.x.as<bf16_t>(), rows, ex, EPI_LOGITS, true);  // (> 64 rows: the wide step's head)
        b = 2.0 * V * HID + act_rw * HID + 2.0 * HID + rows * (V / 8.0);
        break;
      case 5:
        launch_attn_decode_step(aa, s);
        b = (double)rows * c.num_kv_heads * ctx * c.head_dim * 2 * 2 + act_rw * QKV;
        break;
      case 6:
      case 7: {  // QKV with the decode attention fused in (the one-row decode step's form), + o_proj (7)
        const AttnArgs al = X.attn_args(li, rows, e->w.row_slot.as<int>(), e->w.row_pos.as<int>());
        X.qkv_attn_proj(rows, ly, X.fused_attn_args(al, li, which == 7));
        b = 2.0 * QKV * HID + act_rw * (HID + QKV) + 2.0 * HID +
            (double)rows * c.num_kv_heads * ctx * c.head_dim * 2 * 2;
        if (which == 7) b += 2.0 * HID * HD + act_rw * (HD + 2 * HID);
        break;
      }
      case 8:    // the greedy head's int8 screen + exact recheck (lm_head_screen.hip)
      case 9: {  // the screen alone
        X.pending_norm = nullptr;
        X.screened_head_parts(e->w.x.as<bf16_t>(), rows, st, greedy);
        if (which == 8) launch_bump_epoch(st.epoch, s);  // (the step counter finalize advances)
        // int8 matrix + per-column constants + rows + penalty bits (+ the recomputed units' bf16 tiles,
        // a few dozen of 64 KiB, not counted)
        b = (double)V * HID + 16.0 * V + act_rw * HID + rows * (V / 8.0);
        break;
      }
      case 10:    // the sampled step's screened head: screen + exact recompute + the list sampler
      case 11: {  // today's sampling head: the lm_head with the logits store + the dense sampler
        if (which == 10) {
          X.pending_norm = nullptr;
          X.screened_sample(e->w.x.as<bf16_t>(), rows, st, sampled);
          // (+ the recomputed units' bf16 tiles and the candidate lists, not counted)
          b = (double)V * HID + 16.0 * V + act_rw * HID + rows * (V / 8.0);
        } else {
          X.pending_norm = nullptr;
          X.lm_head_pick(e->w.x.as<bf16_t>(), rows, sx, EPI_LOGITS, true);
          SampleArgs sa = X.sample_args(st, sampled, false, X.head_parts(rows, EPI_LOGITS, true));
          sa.out_part_val = nullptr; sa.out_part_idx = nullptr;  // (not the partials: the next launch's
          sa.tokens = e->w.row_idx.as<int>();                    //  bound reads them)
          launch_sample(sa, rows, s);
          // the logits written once and read once by the sampler
          b = 2.0 * V * HID + act_rw * HID + 2.0 * HID + rows * (V / 8.0) + 2.0 * rows * V * 4.0;
        }
        launch_bump_epoch(st.epoch, s);
        break;
      }
      case 12:  // the warm role as a launch of its own (TTS_WARM_STAGES = 0: none), then gate/up
        launch_warm_probe(X.warm_args(ly.wgu, 0), s);
        X.gate_up(rows, ly);
        b = 2.0 * 2 * FF * HID + act_rw * (HID + FF) + 2.0 * HID;
        break;
    }
  };
  launch();
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(e->ev[2], s));
  for (int i = 0; i < iters; ++i) launch();
  HIP_CHECK(hipEventRecord(e->ev[3], s));
  HIP_CHECK(hipEventSynchronize(e->ev[3]));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, e->ev[2], e->ev[3]));
  *avg_ms = ms / iters;
  *bytes = b;
  read_device_flags(e, s);
}

static float bf16_to_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

void lm_score(Engine* e, const int32_t* ids, const int32_t* lens, int B, int n_last,
              float* logits, hipStream_t s) {
  TTS_REQUIRE(e->lm.loaded, "tts_lm_load has not been called");
  TTS_REQUIRE(B >= 1 && B <= e->w.cap_batch, "batch out of range");
  Ctx X(e, s);
  const tts_lm_config& c = X.c;
  for (int b = 0; b < B; ++b) {
    TTS_REQUIRE(lens[b] >= n_last && lens[b] <= c.max_seq_len, "bad sequence length");
  }
  const std::vector<int> last_rows = X.prefill_group(ids, lens, B, 0);
  // gather the last n_last rows of every sequence
  std::vector<int> sel;
  for (int b = 0; b < B; ++b)
    for (int i = n_last - 1; i >= 0; --i) sel.push_back(last_rows[b] - i);
  const int nsel = (int)sel.size();
  DevBuf sel_d, xs, lg;
  sel_d.alloc(nsel * 4);
  xs.alloc((size_t)nsel * c.hidden_size * 2);
  lg.alloc((size_t)nsel * c.vocab_size * 2);
  HIP_CHECK(hipMemcpyAsync(sel_d.p, sel.data(), nsel * 4, hipMemcpyHostToDevice, s));
  launch_gather_rows(e->w.x.as<bf16_t>(), c.hidden_size, sel_d.as<int>(), xs.as<bf16_t>(), nsel,
                     c.hidden_size, s);
  // the lm_head in launches of <= kPrefillChunk rows: the decode GEMM's K order, which the
  // step's first token (B <= 64 gathered rows) also takes, so a sequence's logits do not depend
  // on how many sequences are scored with it (the prefill GEMM sums K in 1024-chunks)
  for (int r0 = 0; r0 < nsel; r0 += kPrefillChunk)
    X.lm_head_logits(xs.as<bf16_t>() + (size_t)r0 * c.hidden_size, std::min(kPrefillChunk, nsel - r0),
                     lg.as<bf16_t>() + (size_t)r0 * c.vocab_size);
  HIP_CHECK(hipGetLastError());
  std::vector<uint16_t> h((size_t)nsel * c.vocab_size);
  HIP_CHECK(hipMemcpyAsync(h.data(), lg.p, h.size() * 2, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (size_t i = 0; i < h.size(); ++i) logits[i] = bf16_to_f32(h[i]);
}

// Teacher forcing through the DECODE step's kernels (the path generate runs after prefill):
// prefill the first lens[b] - n_last tokens of every sequence, then feed the remaining
// n_last tokens one decode step at a time (all rows together, the step's launch sequence:
// fused QKV+attention(+o_proj) at one row, the batched GEMVs and the (row, kv head) decode
// attention otherwise) and keep each step's bf16 logits.  Same positions as lm_score, so
// the two differ only by prefill vs decode arithmetic.  gidx (optional, [B][n_last][k]):
// keep only those vocabulary entries; otherwise k = V.
void lm_score_decode(Engine* e, const int32_t* ids, const int32_t* lens, int B, int n_last,
                     const int32_t* gidx, int k, float* out, hipStream_t s) {
  TTS_REQUIRE(e->lm.loaded, "tts_lm_load has not been called");
  TTS_REQUIRE(B >= 1 && B <= e->w.cap_batch, "batch out of range");
  Ctx X(e, s);
  const tts_lm_config& c = X.c;
  const int V = c.vocab_size, HID = c.hidden_size;
  if (!gidx) k = V;
  TTS_REQUIRE(k >= 1 && k <= V, "bad gather width");
  std::vector<int> start(B), plen(B);
  for (int b = 0, off = 0; b < B; off += lens[b], ++b) {
    TTS_REQUIRE(lens[b] > n_last && lens[b] <= c.max_seq_len, "bad sequence length (needs lens > n_last)");
    start[b] = off;
    plen[b] = lens[b] - n_last;
  }
  if (gidx)
    for (size_t i = 0; i < (size_t)B * n_last * k; ++i) TTS_REQUIRE(gidx[i] >= 0 && gidx[i] < V, "gather index out of range");
  // ---- prefill the prefixes (groups of whole prefixes that fit the workspace)
  X.prefill_all(ids, start, plen, false, "prefix");
  // ---- n_last decode steps with the given tokens
  std::vector<int> tok(B), pos(B);
  DevBuf lg;
  lg.alloc((size_t)B * V * 2);
  std::vector<uint16_t> h((size_t)B * V);
  X.upload_identity_slots(B);
  for (int i = 0; i < n_last; ++i) {
    for (int b = 0; b < B; ++b) {
      tok[b] = ids[start[b] + plen[b] + i];
      pos[b] = plen[b] + i;
    }
    HIP_CHECK(hipMemcpyAsync(e->w.row_idx.p, tok.data(), B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(e->w.row_pos.p, pos.data(), B * 4, hipMemcpyHostToDevice, s));
    launch_embed(e->w.row_idx.as<int>(), X.M.embed_rows.as<bf16_t>(), e->w.x.as<bf16_t>(), B, HID, s);
    X.layers(B, e->w.row_slot.as<int>(), e->w.row_pos.as<int>(), true);
    X.lm_head_logits(e->w.x.as<bf16_t>(), B, lg.as<bf16_t>());
    launch_bump_epoch(e->w.epoch.as<uint32_t>(), s);  // (a decode step without the finalize kernel)
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h.data(), lg.p, h.size() * 2, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (h and the token/position vectors are reused)
    for (int b = 0; b < B; ++b) {
      float* o = out + ((size_t)b * n_last + i) * k;
      const uint16_t* hb = h.data() + (size_t)b * V;
      const int32_t* gi = gidx ? gidx + ((size_t)b * n_last + i) * k : nullptr;
      for (int j = 0; j < k; ++j) o[j] = bf16_to_f32(hb[gi ? gi[j] : j]);
    }
  }
  read_device_flags(e, s);
}

}  // namespace tts
