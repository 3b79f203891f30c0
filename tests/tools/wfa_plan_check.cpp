// tests/tools/wfa_plan_check.cpp -- the launch plan of the alignment kernels (trgt_amd/csrc/wfa_plan.hpp) held to its invariants on a
// sweep of inputs, to the routes of the launches the project makes, and to the error of every launch it refuses.  No GPU, no HIP:
//   g++ -std=c++17 -I include tests/tools/wfa_plan_check.cpp -o wfa_plan_check && ./wfa_plan_check
// (tests/test_wfa_plan.py does that; with -fsanitize=address,undefined the narrowings of the layout are checked too).  Prints one
// "plan <row> ..." line per pinned row -- tests/test_wfa_launch_errors_gpu.py reads ws_per_block of the workspace-limit rows -- and
// exits 0 when everything held.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../trgt_amd/csrc/wfa_plan.hpp"

using namespace trgt;

static int g_failed = 0;
static std::string g_row;
#define CHECK(cond) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s: %s (line %d)\n", g_row.c_str(), #cond, __LINE__); } } while (0)

static trgt_wfa_params params(int metric, int x, int o, int e, int span, int tbf, int tef, int scope, int memory, int heuristic) {
  trgt_wfa_params p;
  std::memset(&p, 0, sizeof p);
  p.metric = metric; p.mismatch = x; p.gap_open1 = o; p.gap_ext1 = e; p.gap_open2 = 24; p.gap_ext2 = 1;
  p.span = span; p.text_begin_free = tbf; p.text_end_free = tef; p.scope = scope; p.memory_mode = memory; p.heuristic = heuristic;
  p.h_min_wavefront_length = 10; p.h_max_distance_threshold = 50; p.h_steps_between_cutoffs = 1;  // (trgt_wfa_default_params)
  p.bialign_min_score = 250; p.bialign_min_length = 100;
  return p;
}
static WfaPlanIn input(const trgt_wfa_params& p, int64_t n_jobs, int64_t mp, int64_t mt, int threads) {
  WfaPlanIn in;
  in.p = p; in.n_jobs_host = n_jobs; in.max_plen = mp; in.max_tlen = mt; in.max_sum = mp + mt; in.threads = threads;
  return in;
}

static bool pow2(uint64_t v) { return v && !(v & (v - 1)); }

// what every plan that stands must satisfy
static void invariants(const WfaPlanIn& in, const WfaPlan& q) {
  const bool biwfa = in.p.memory_mode == 3;
  // the workspace: ascending, 256-aligned pieces that do not overlap and end at ws_per_block
  const uint64_t ring_bytes = biwfa ? 4ull * (uint64_t)q.pen.scope * (uint64_t)q.pen.ncomp * q.ring_stride : 0;
  const uint64_t off[8] = {q.off_gdesc, q.off_arena_u, q.off_arena_f, q.off_arena_r, q.off_rle_tmp, q.off_rle_out, q.off_run_start, q.ws_per_block};
  const uint64_t need[7] = {(uint64_t)q.uni_slots * 5 * sizeof(wfa::WfDesc), 4ull * q.arena_uni_cap, ring_bytes, ring_bytes, 4ull * q.rle_cap, 4ull * q.rle_cap, 4ull * q.rle_cap};
  CHECK(off[0] == 0);
  for (int i = 0; i < 7; ++i) { CHECK(off[i] % 256 == 0); CHECK(off[i] <= off[i + 1]); CHECK(off[i] + need[i] <= off[i + 1]); }
  CHECK(q.ws_per_block % 256 == 0);
  CHECK((int64_t)q.uni_slots == q.score_bound + 1 && (int64_t)q.rle_cap == in.max_sum + 4 && (int64_t)q.ring_stride == in.max_sum + 4);  // nothing lost in the narrowings
  CHECK(q.arena_uni_cap >= 64);
  // workgroups
  CHECK(q.blocks >= 1);
  CHECK((uint64_t)q.blocks * q.ws_per_block <= in.ws_limit);
  if (in.ws_budget > 0 && q.blocks > 1) CHECK((uint64_t)q.blocks * q.ws_per_block <= in.ws_budget);
  CHECK(q.blocks <= std::max<int64_t>(in.n_jobs_host, 1));
  CHECK(q.counter_bytes == 16 + 4 * (uint64_t)q.blocks + 160);
  CHECK(q.threads > 0 && q.jobs_bound == (in.jobs_bound > 0 ? in.jobs_bound : in.n_jobs_host));
  // routes: exactly one main route, at most one front route and that only in front of the generic kernel
  CHECK(q.main == WFA_MAIN_FAST || q.main == WFA_MAIN_GENERIC);
  CHECK((q.main == WFA_MAIN_FAST) == (q.fast_wcap > 0));
  CHECK(q.front == WFA_FRONT_NONE || q.front == WFA_FRONT_LEAN || q.front == WFA_FRONT_ARENA);
  if (q.front != WFA_FRONT_NONE) CHECK(q.main == WFA_MAIN_GENERIC && biwfa && q.threads == 64 && !in.has_ops);
  const uint64_t staged = ((uint64_t)in.max_plen + 15) / 16 * 16 + (uint64_t)in.max_tlen + 16;
  CHECK((q.lds_seq_cap == 0) == (staged > 32 * 1024 || in.wfa_no_stage));
  if (q.lds_seq_cap) CHECK(q.lds_seq_cap >= staged && q.lds_seq_cap % 16 == 0);
  if (q.main == WFA_MAIN_FAST) {
    const uint64_t window = 4ull * (uint64_t)(in.max_plen + in.max_tlen + 8);
    CHECK(q.main_id >= 0 && q.main_id < WFA_FAST_IDS);
    CHECK(q.lds == (uint64_t)q.fast_ring_bytes + window && q.lds <= 96 * 1024);
    CHECK(in.max_tlen + q.score_bound < 65000);
    CHECK(q.ring_mask == 0 && q.ring_off == 0 && q.lds_seq_cap > 0);
    CHECK(in.p.metric == 3 && in.p.heuristic == 0 && !biwfa && q.threads % 64 == 0 && q.threads <= 256);
    CHECK((q.fast_koff != 0) == q.capped);
  } else {
    CHECK(q.main_id >= 0 && q.main_id < WFA_GENERIC_IDS && (q.main_id < 5 ? q.main_id == in.p.metric : in.p.metric == (q.main_id == 5 ? 1 : 3)));
    CHECK(q.ring_mask == wfa::RING - 1 && q.ring_off >= q.lds_seq_cap && q.ring_off % 16 == 0);
    CHECK(q.lds == q.ring_off + 3ull * wfa::RING * 5 * sizeof(wfa::WfDesc));
    CHECK(q.fast_ring_bytes == 0 && q.fast_wcap == 0);
  }
  if (q.front == WFA_FRONT_ARENA) {
    CHECK(pow2((uint64_t)q.la_ring_mask + 1) && (int)(q.la_ring_mask + 1) >= q.pen.scope);
    CHECK(q.arena_id >= 0 && q.arena_id < 4);
    CHECK(q.la_rle_tmp == q.la_seq_cap && q.la_rle_out == q.la_rle_tmp + 4 * q.la_rle_cap && q.la_ring_off == q.la_rle_out + 4 * q.la_rle_cap);
    CHECK(q.la_region == q.la_ring_off + 3 * (q.la_ring_mask + 1) * 5 * sizeof(wfa::WfDesc) && q.la_lds == (uint64_t)q.la_region + q.la_region_bytes);
    CHECK(q.la_gdesc_slots >= 1 && 3ull * q.la_gdesc_slots * 5 * sizeof(wfa::WfDesc) <= q.la_region_bytes);
  } else CHECK(q.la_lds == 0);
  CHECK(q.pen.scope >= 2 && q.pen.scope <= wfa::RING);
}

static int plan_row(const char* name, const WfaPlanIn& in, WfaPlan* q, const char** why) {
  g_row = name;
  *why = "";
  const int rc = wfa_plan(in, q, why);
  if (rc == TRGT_OK) invariants(in, *q);
  return rc;
}

// a pinned launch: must plan, and take this route
static WfaPlan pinned(const char* name, const WfaPlanIn& in, WfaMainRoute main, int main_id, WfaFrontRoute front) {
  WfaPlan q; const char* why;
  const int rc = plan_row(name, in, &q, &why);
  std::printf("plan %s rc=%d main=%d.%d front=%d threads=%d blocks=%" PRId64 " score_bound=%" PRId64 " ws_per_block=%" PRIu64 " lds=%" PRIu64 " fast_koff=%u\n", name, rc, (int)q.main, q.main_id,
              (int)q.front, q.threads, q.blocks, q.score_bound, q.ws_per_block, q.lds, q.fast_koff);
  CHECK(rc == TRGT_OK);
  CHECK(q.main == main && q.main_id == main_id && q.front == front);
  return q;
}

// a launch that must be refused with this code and a message that holds `text`
static WfaPlan refused(const char* name, const WfaPlanIn& in, int code, const char* text) {
  WfaPlan q; const char* why;
  const int rc = plan_row(name, in, &q, &why);
  std::printf("plan %s rc=%d ws_per_block=%" PRIu64 " why=%s\n", name, rc, q.ws_per_block, why);
  CHECK(rc == code);
  CHECK(std::strstr(why, text) != nullptr);
  return q;
}

// ---- every metric, span, memory mode, scope and thread count over short, odd, long and very long pairs, small and large workspaces
static void sweep() {
  const int64_t lens[][2] = {{0, 0}, {1, 0}, {0, 9}, {13, 17}, {250, 850}, {250, 3000}, {250, 40000}, {2000, 2000}, {16384, 16368}, {16384, 16369}, {20000, 30000},
                             {70000, 70000}, {1 << 20, 1 << 20}, {(1 << 26) - 1, 1 << 26}, {1 << 26, 1 << 26}};
  const int pens[][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, 6, 0, 2}, {2, 31, 0, 1}, {3, 2, 5, 1}, {3, 1, 0, 1}, {3, 7, 9, 1}, {3, 4, 25, 2}, {4, 8, 4, 2}, {4, 4, 2, 3}};
  const int spans[][3] = {{0, 0, 0}, {1, -1, -1}, {1, 40, 7}, {1, 70, -1}};
  const int threads[] = {0, 64, 128, 192, 256, 512};
  const uint64_t limits[] = {32ull << 30, 8ull << 30, 3ull << 20};
  int64_t stood = 0, refused_n = 0;
  char name[160];
  for (const auto& len : lens) for (const auto& pe : pens) for (const auto& sp : spans) for (int memory : {0, 3}) for (int scope : {0, 1}) for (int th : threads)
    for (uint64_t limit : limits) for (int variant = 0; variant < 6; ++variant) {
      if (memory == 3 && sp[0] != 0) continue;  // (refused: its own row below)
      WfaPlanIn in = input(params(pe[0], pe[1], pe[2], pe[3], sp[0], sp[1], sp[2], scope, memory, variant & 1), 1 + 977 * (variant + 1) * (th + 1) % 5000, len[0], len[1], th);
      in.ws_limit = limit;
      in.num_cus = variant == 2 ? 1 : 256;
      if (variant == 1) { in.ws_budget = 512ull << 20; in.has_n_jobs_dev = true; in.jobs_bound = 100000; }
      if (variant == 2) { in.no_lean = true; in.no_lds_wfa = false; in.lds_wfa_kb = 3; in.wfa_no_stage = true; }
      if (variant == 3) { in.no_lean = true; in.no_lds_wfa = false; in.lds_wfa_kb = 18; in.lds_wfa_seq = 100; in.wfa_no_wave_variant = true; }
      if (variant == 4) { in.max_score = 15; in.tag = 2; in.no_spec = len[0] & 1; }
      if (variant == 5) { in.has_ops = true; in.has_jobs2 = true; in.tag = 1; in.max_score = 96; }
      std::snprintf(name, sizeof name, "sweep p=%" PRId64 " t=%" PRId64 " metric=%d pen=%d,%d,%d span=%d,%d,%d memory=%d scope=%d threads=%d limit=%" PRIu64 " variant=%d", len[0], len[1], pe[0], pe[1], pe[2], pe[3],
                    sp[0], sp[1], sp[2], memory, scope, th, limit, variant);
      WfaPlan q; const char* why;
      const int rc = plan_row(name, in, &q, &why);
      if (rc == TRGT_OK) ++stood;
      else { ++refused_n; CHECK(rc == TRGT_ERR_NOMEM && std::strstr(why, "workspace")); }  // (the sweep's parameters are valid: only the limit refuses)
    }
  g_row = "sweep";
  std::printf("sweep: %" PRId64 " plans stood, %" PRId64 " refused for the workspace limit\n", stood, refused_n);
  CHECK(stood > 20000 && refused_n > 1000);
}

// ---- the launches the project makes (spans.hip: SpanCall; locus.hip: the consensus repair and the cluster chain)
static void routes() {
  const trgt_wfa_params flank = params(3, 2, 5, 1, 1, -1, -1, 1, 0, 0);  // THREAD_WFA_FLANK: pattern global, text free
  for (int th : {256, 192}) {
    WfaPlanIn in = input(flank, 100000, 250, 3000, th);
    in.tag = 1; in.has_n_jobs_dev = true; in.has_jobs2 = true;
    pinned(th == 256 ? "flank_rest_256" : "flank_rest_192", in, WFA_MAIN_FAST, (th == 256 ? WFA_FAST_256_T0 : WFA_FAST_192_T0) + 1, WFA_FRONT_NONE);
    in.no_spec = true;
    pinned(th == 256 ? "flank_rest_256_no_spec" : "flank_rest_192_no_spec", in, WFA_MAIN_FAST, WFA_FAST_ANY_T0 + 1, WFA_FRONT_NONE);
  }
  {  // the windowed launch: eight segments of a 250-base piece, S0 = 15, windows of 320 bases started on 71 diagonals
    trgt_wfa_params w = flank; w.text_begin_free = 70;
    WfaPlanIn in = input(w, 100000, 250, 320, 64);
    in.tag = 2; in.max_score = 15; in.has_n_jobs_dev = true;
    const WfaPlan q = pinned("windowed_64", in, WFA_MAIN_FAST, WFA_FAST_64_T2, WFA_FRONT_NONE);
    CHECK(q.fast_koff == 15 + 4 && q.score_bound == 16);
  }
  for (int th : {64, 128, 256}) {  // the banded back-trace of what the pre-filter keeps: s* <= 96, texts of 250 + 2 * 96
    trgt_wfa_params w = flank; w.text_begin_free = 192;
    WfaPlanIn in = input(w, 100000, 250, 442, th);
    in.tag = 3; in.max_score = 96; in.has_n_jobs_dev = true;
    const WfaPlan q = pinned(th == 64 ? "banded_64" : th == 128 ? "banded_128" : "banded_256", in, WFA_MAIN_FAST, th == 64 ? WFA_FAST_64_T3 : th == 128 ? WFA_FAST_128_T3 : WFA_FAST_256_T3, WFA_FRONT_NONE);
    CHECK(q.fast_koff == 100);
  }
  const trgt_wfa_params cons = params(3, 2, 5, 1, 0, 0, 0, 1, 3, 1);  // THREAD_WFA_CONSENSUS: BiWFA, (2,5,1), default heuristic
  const trgt_wfa_params ed = params(1, 0, 0, 0, 0, 0, 0, 0, 3, 1);    // THREAD_WFA_ED: edit distance, score only, BiWFA
  for (int which = 0; which < 2; ++which) {
    WfaPlanIn in = input(which ? ed : cons, 128, 4096, 4096, 0);
    in.has_n_jobs_dev = true; in.jobs_bound = 50000; in.buffer_set = 2; in.ws_budget = 512ull << 20;
    const int wave_id = wfa_generic_id(in.p.metric, true), plain_id = wfa_generic_id(in.p.metric, false);
    CHECK(wave_id != plain_id);
    WfaPlan q = pinned(which ? "edit_distances" : "consensus", in, WFA_MAIN_GENERIC, wave_id, WFA_FRONT_LEAN);
    CHECK(q.threads == 64 && q.jobs_bound == 50000 && (uint64_t)q.blocks * q.ws_per_block <= (512ull << 20));
    in.no_lean = true;
    pinned(which ? "edit_distances_no_lean" : "consensus_no_lean", in, WFA_MAIN_GENERIC, wave_id, WFA_FRONT_NONE);
    in.no_lds_wfa = false;
    q = pinned(which ? "edit_distances_arena" : "consensus_arena", in, WFA_MAIN_GENERIC, wave_id, WFA_FRONT_ARENA);
    CHECK(q.arena_id == wfa_arena_id(in.p.metric, true) && q.la_ring_mask + 1 == (which ? 2u : 8u));
    in.wfa_no_wave_variant = true;
    q = pinned(which ? "edit_distances_arena_no_wave" : "consensus_arena_no_wave", in, WFA_MAIN_GENERIC, plain_id, WFA_FRONT_ARENA);
    CHECK(q.arena_id == wfa_arena_id(in.p.metric, false));
    in.no_lean = false; in.no_lds_wfa = true;
    pinned(which ? "edit_distances_no_wave" : "consensus_no_wave", in, WFA_MAIN_GENERIC, plain_id, WFA_FRONT_LEAN);
    in.wfa_no_wave_variant = false; in.has_ops = true;
    pinned(which ? "edit_distances_ops" : "consensus_ops", in, WFA_MAIN_GENERIC, wave_id, WFA_FRONT_NONE);
  }
  {  // a pair too long for 96 KB of LDS: the generic kernel, the short pairs of the batch with it
    WfaPlanIn in = input(params(3, 2, 5, 1, 0, 0, 0, 1, 0, 0), 15, 2000, 2010, 64);
    in.has_ops = true;
    pinned("too_long_for_lds", in, WFA_MAIN_GENERIC, wfa_generic_id(3, true), WFA_FRONT_NONE);
    in.max_plen = 300; in.max_tlen = 310; in.max_sum = 610;
    pinned("fits_lds", in, WFA_MAIN_FAST, WFA_FAST_ANY_T0, WFA_FRONT_NONE);
  }
}

// ---- every launch wfa_launch refuses
static void refusals() {
  const trgt_wfa_params ok = params(3, 2, 5, 1, 0, 0, 0, 1, 0, 0);
  trgt_wfa_params p = ok; p.metric = 5;
  refused("bad_metric", input(p, 2, 50, 50, 0), TRGT_ERR_INVALID, "wfa: bad metric 5");
  p = ok; p.metric = -1;
  refused("negative_metric", input(p, 2, 50, 50, 0), TRGT_ERR_INVALID, "wfa: bad metric -1");
  p = ok; p.heuristic = 2;
  refused("heuristic_2", input(p, 2, 50, 50, 0), TRGT_ERR_UNSUPPORTED, "only Heuristic::None and WFadaptive");
  p = ok; p.memory_mode = 3; p.span = 1;
  refused("biwfa_with_a_span", input(p, 2, 50, 50, 0), TRGT_ERR_UNSUPPORTED, "BiWFA is end-to-end only");
  p = ok; p.mismatch = 0;
  refused("zero_mismatch", input(p, 2, 50, 50, 0), TRGT_ERR_INVALID, "penalties must be positive");
  p = ok; p.gap_ext1 = 0;
  refused("zero_extension", input(p, 2, 50, 50, 0), TRGT_ERR_INVALID, "penalties must be positive");
  p = ok; p.gap_open1 = -1;
  refused("negative_opening", input(p, 2, 50, 50, 0), TRGT_ERR_INVALID, "penalties must be positive");
  refused("score_scope_33", input(params(2, 32, 0, 1, 0, 0, 0, 1, 0, 0), 2, 50, 50, 0), TRGT_ERR_UNSUPPORTED, "score scope of 33 (> 32)");
  { WfaPlan q; const char* why; CHECK(plan_row("score_scope_32", input(params(2, 31, 0, 1, 0, 0, 0, 1, 0, 0), 2, 50, 50, 0), &q, &why) == TRGT_OK && q.pen.scope == 32); }
  refused("score_scope_41", input(params(3, 40, 6, 2, 0, 0, 0, 1, 0, 0), 2, 50, 50, 0), TRGT_ERR_UNSUPPORTED, "score scope of 41 (> 32)");
  WfaPlanIn in = input(ok, 100, 250, 442, 64);  // tag 3 outside the flank configuration: end to end, and (2,5,1) text-free without a score cap
  in.tag = 3; in.max_score = 96;
  refused("banded_end_to_end", in, TRGT_ERR_INVALID, "banded launch exists for the flank configuration only");
  in = input(params(3, 2, 5, 1, 1, -1, -1, 1, 0, 0), 100, 250, 442, 64);
  in.tag = 3;
  refused("banded_without_a_cap", in, TRGT_ERR_INVALID, "banded launch exists for the flank configuration only");
  in.p.text_begin_free = 192; in.max_score = 96; in.threads = 192;
  refused("banded_192_threads", in, TRGT_ERR_INVALID, "banded launch exists for the flank configuration only");
  in.threads = 64; in.tag = 4;
  refused("kernel_tag_4", in, TRGT_ERR_INVALID, "no kernel tag 4");
  in = input(params(3, 2, 5, 1, 0, 0, 0, 1, 3, 1), 64, 300, 300, 0);  // the lean route with a device-side job count
  in.has_n_jobs_dev = true;
  refused("device_count_without_jobs_bound", in, TRGT_ERR_INVALID, "needs jobs_bound");
  in.jobs_bound = 64;
  pinned("device_count_with_jobs_bound", in, WFA_MAIN_GENERIC, wfa_generic_id(3, true), WFA_FRONT_LEAN);
  in.jobs_bound = 0; in.no_lean = true;
  pinned("device_count_no_lean", in, WFA_MAIN_GENERIC, wfa_generic_id(3, true), WFA_FRONT_NONE);
  // both workspace-limit messages: an edit-distance, full-history batch of two pairs of 2 000 bases
  in = input(params(1, 0, 0, 0, 0, 0, 0, 1, 0, 1), 2, 2000, 2000, 0);
  in.has_ops = true;
  in.ws_limit = 4096;
  refused("workspace_limit_4096", in, TRGT_ERR_NOMEM, "wfa: workspace limit 4096 B too small");
  in.ws_limit = 1 << 20;
  const WfaPlan q = refused("workspace_limit_1mib", in, TRGT_ERR_NOMEM, "wfa: one workgroup needs ");
  char want[160];
  std::snprintf(want, sizeof want, "wfa: one workgroup needs %" PRIu64 " B of workspace, limit is 1048576 B", q.ws_per_block);
  CHECK(std::strcmp(q.msg, want) == 0 && q.ws_per_block > (1u << 20));
  in.ws_limit = 32ull << 30;
  const WfaPlan r = pinned("workspace_limit_default", in, WFA_MAIN_GENERIC, wfa_generic_id(1, true), WFA_FRONT_NONE);
  CHECK(r.ws_per_block == q.ws_per_block && r.blocks == 2);
}

int main() {
  sweep();
  routes();
  refusals();
  if (g_failed) { std::printf("%d checks FAILED\n", g_failed); return 1; }
  std::printf("wfa_plan_check: all held\n");
  return 0;
}
