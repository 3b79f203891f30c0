// trgt_amd/csrc/wfa_plan.hpp -- what wfa_launch (wfa.hip) decides before it touches the device, as one pure function of plain values:
// the penalty record, the score bound, the layout of a workgroup's HBM workspace, the kernel that runs (and the one in front of it), and
// the LDS of each.  No HIP here: tests/tools/wfa_plan_check.cpp compiles it with the host compiler and holds it to its invariants.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/trgt_hip.h"
#include "wfa_types.hpp"

namespace trgt {

struct WfaPlanIn {
  trgt_wfa_params p;
  // of the WfaLaunch (wfa_host.hpp)
  int64_t n_jobs_host = 0, jobs_bound = 0, max_plen = 0, max_tlen = 0, max_sum = 0;
  int threads = 0, max_score = 0;
  int tag = 0;  // kernel_tag, resolved (0 .. 3)
  uint64_t ws_budget = 0;
  int buffer_set = 0;
  bool has_ops = false, has_n_jobs_dev = false, has_jobs2 = false;  // expanded operations wanted; a device-side job count; a second list part
  // of the context
  int num_cus = 256;
  uint64_t ws_limit = 32ull << 30;
  bool no_spec = false, no_lean = false, no_lds_wfa = true, wfa_no_wave_variant = false, wfa_no_stage = false, skip_bt = false;
  int lds_wfa_seq = 768, lds_wfa_kb = 7;
};

// The main launch: the dedicated LDS-resident kernel (wfa_fast.hpp) when every job of the batch qualifies, else the generic one.
enum WfaMainRoute { WFA_MAIN_FAST = 0, WFA_MAIN_GENERIC = 1 };
// instantiations of the dedicated kernel, thread specialisation (ANY: none) x kernel tag: the flank specialisations and the general one
// take tags 0 .. 2 (id = its tag 0 + tag), the banded launches (tag 3) and the windowed one (64 threads, tag 2) have their own
enum WfaFastId { WFA_FAST_256_T0 = 0, WFA_FAST_192_T0 = 3, WFA_FAST_ANY_T0 = 6, WFA_FAST_256_T3 = 9, WFA_FAST_128_T3, WFA_FAST_64_T3, WFA_FAST_64_T2, WFA_FAST_IDS };
// ... of the generic kernel: the workgroup build of metric 0 .. 4, then the one-wave builds that edit (1) and gap-affine (3) have
constexpr int WFA_GENERIC_IDS = 7;
constexpr int wfa_generic_id(int metric, bool wave) { return wave ? (metric == 1 ? 5 : 6) : metric; }
// BiWFA batches of one wave per alignment (consensus alignments, edit distances) go through a kernel in front of the generic one, which
// then redoes what that one hands on: the register-resident tiers (wfa_lean.hip), or the LDS-arena variant of the generic kernel
enum WfaFrontRoute { WFA_FRONT_NONE = 0, WFA_FRONT_LEAN = 1, WFA_FRONT_ARENA = 2 };
// instantiations of the LDS-arena variant: (workgroup build, one-wave build) x (edit, gap-affine)
constexpr int wfa_arena_id(int metric, bool wave) { return (wave ? 2 : 0) + (metric == 3 ? 1 : 0); }

struct WfaPlan {
  wfa::Pen pen;
  int64_t score_bound = 0;
  bool capped = false;  // max_score bounds the levels (and with them the diagonals) of every job
  // a workgroup's piece of the HBM workspace
  uint64_t off_gdesc = 0, off_arena_u = 0, off_arena_f = 0, off_arena_r = 0, off_rle_tmp = 0, off_rle_out = 0, off_run_start = 0, ws_per_block = 0;
  uint32_t uni_slots = 0, arena_uni_cap = 0, ring_stride = 0, rle_cap = 0;
  int threads = 0;
  int64_t blocks = 0;  // most workgroups that can be resident (one workspace piece each); the launch applies the occupancy to it
  int64_t jobs_bound = 0;
  uint64_t counter_bytes = 0;
  // main launch
  WfaMainRoute main = WFA_MAIN_GENERIC;
  int main_id = 0;  // WfaFastId / wfa_generic_id
  uint32_t lds_seq_cap = 0, fast_wcap = 0, fast_ring_bytes = 0, fast_koff = 0, fast_dbg = 0, ring_off = 0, ring_mask = 0;
  uint64_t lds = 0;  // dynamic LDS of the main launch
  // front launch
  WfaFrontRoute front = WFA_FRONT_NONE;
  int arena_id = 0;
  uint32_t la_seq_cap = 0, la_rle_tmp = 0, la_rle_out = 0, la_rle_cap = 0, la_ring_off = 0, la_ring_mask = 0, la_region = 0, la_region_bytes = 0, la_gdesc_slots = 0;
  uint64_t la_lds = 0;
  char msg[192] = {0};  // why the plan failed
};

inline int wfa_gap_cost(const trgt_wfa_params& p, int64_t len) {
  if (len <= 0) return 0;
  int64_t c;
  switch (p.metric) {
    case 0: case 1: c = len; break;
    case 2: c = (int64_t)p.gap_ext1 * len; break;
    case 3: c = p.gap_open1 + (int64_t)p.gap_ext1 * len; break;
    default: c = std::min<int64_t>(p.gap_open1 + (int64_t)p.gap_ext1 * len, p.gap_open2 + (int64_t)p.gap_ext2 * len); break;
  }
  return (int)std::min<int64_t>(c, 1 << 28);
}

namespace wfa_plan_detail {
__attribute__((format(printf, 4, 5))) inline int refuse(WfaPlan* q, const char** why, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(q->msg, sizeof q->msg, fmt, ap);
  va_end(ap);
  if (why) *why = q->msg;
  return code;
}
inline uint64_t al256(uint64_t v) { return (v + 255) & ~255ull; }

inline int plan_penalties(const trgt_wfa_params& p, WfaPlan* q, const char** why) {
  if (p.metric < 0 || p.metric > 4) return refuse(q, why, TRGT_ERR_INVALID, "wfa: bad metric %d", p.metric);
  if (p.heuristic != 0 && p.heuristic != 1) return refuse(q, why, TRGT_ERR_UNSUPPORTED, "wfa: only Heuristic::None and WFadaptive are implemented");
  if (p.memory_mode == 3 && p.span != 0) return refuse(q, why, TRGT_ERR_UNSUPPORTED, "wfa: BiWFA is end-to-end only (as used by TRGT)");
  if (p.metric >= 2 && (p.mismatch <= 0 || p.gap_ext1 <= 0 || (p.metric >= 3 && p.gap_open1 < 0)))
    return refuse(q, why, TRGT_ERR_INVALID, "wfa: penalties must be positive");
  wfa::Pen& pen = q->pen;
  pen.metric = p.metric;
  switch (p.metric) {
    case 0: pen.x = -1; pen.o1 = 1; pen.e1 = -1; pen.o2 = pen.e2 = -1; pen.scope = 2; pen.ncomp = 1; break;
    case 1: pen.x = 1; pen.o1 = 1; pen.e1 = -1; pen.o2 = pen.e2 = -1; pen.scope = 2; pen.ncomp = 1; break;
    case 2: pen.x = p.mismatch; pen.o1 = p.gap_ext1; pen.e1 = -1; pen.o2 = pen.e2 = -1; pen.scope = std::max(pen.x, pen.o1) + 1; pen.ncomp = 1; break;
    case 3: pen.x = p.mismatch; pen.o1 = p.gap_open1; pen.e1 = p.gap_ext1; pen.o2 = pen.e2 = -1; pen.scope = std::max(pen.x, pen.o1 + pen.e1) + 1; pen.ncomp = 3; break;
    default: pen.x = p.mismatch; pen.o1 = p.gap_open1; pen.e1 = p.gap_ext1; pen.o2 = p.gap_open2; pen.e2 = p.gap_ext2;
      pen.scope = std::max(pen.x, std::max(pen.o1 + pen.e1, pen.o2 + pen.e2)) + 1; pen.ncomp = 5; break;
  }
  if (pen.scope > wfa::RING) return refuse(q, why, TRGT_ERR_UNSUPPORTED, "wfa: penalties need a score scope of %d (> %d)", pen.scope, wfa::RING);
  return TRGT_OK;
}

// the score bound from the batch maxima, and a workgroup's piece of the workspace sized for it
inline int plan_workspace(const WfaPlanIn& in, WfaPlan* q, const char** why) {
  const trgt_wfa_params& p = in.p;
  const wfa::Pen& pen = q->pen;
  const bool biwfa = p.memory_mode == 3, alignment = p.scope != 0;
  const int64_t mp = in.max_plen, mt = in.max_tlen, msum = in.max_sum;
  int64_t score_bound;
  const bool text_free = p.span == 1 && (p.text_begin_free < 0) && (p.text_end_free < 0);
  if (text_free) score_bound = wfa_gap_cost(p, mp) + 2;          // delete the whole pattern anywhere in the free text
  else score_bound = (int64_t)wfa_gap_cost(p, mp) + wfa_gap_cost(p, mt) + 2;
  if (biwfa && alignment) {                                   // base cases: score <= 250 unless the heuristic misleads; min-length fallback
    const int64_t small = (int64_t)wfa_gap_cost(p, std::min<int64_t>(mp, p.bialign_min_length)) + wfa_gap_cost(p, std::min<int64_t>(mt, p.bialign_min_length)) + 2;
    score_bound = std::min<int64_t>(score_bound, std::max<int64_t>(small, 4 * (int64_t)p.bialign_min_score + 64));
  }
  score_bound = std::min<int64_t>(score_bound, 1 << 20);
  q->capped = in.max_score > 0 && p.span == 1 && p.pattern_begin_free == 0 && p.text_begin_free >= 0;
  if (q->capped) score_bound = std::min<int64_t>(score_bound, in.max_score + 1);
  q->score_bound = score_bound;
  const uint64_t per_level = (uint64_t)pen.ncomp * (uint64_t)std::min<int64_t>(msum + 3, 2 * score_bound + 3 + (p.span ? msum : 0));
  const uint64_t arena_ints = std::min<uint64_t>((uint64_t)(score_bound + 1) * per_level + 64, (1ull << 30) / 4);  // <= 1 GiB per workgroup
  const uint64_t ring_stride = (uint64_t)msum + 4;
  const uint64_t ring_ints = biwfa ? (uint64_t)pen.scope * pen.ncomp * ring_stride : 0;
  uint64_t off = 0;
  q->uni_slots = (uint32_t)(score_bound + 1);
  q->off_gdesc = off; off = al256(off + (uint64_t)q->uni_slots * 5 * sizeof(wfa::WfDesc));
  q->off_arena_u = off; off = al256(off + arena_ints * 4);
  q->off_arena_f = off; off = al256(off + ring_ints * 4);
  q->off_arena_r = off; off = al256(off + ring_ints * 4);
  q->rle_cap = (uint32_t)(msum + 4);
  q->off_rle_tmp = off; off = al256(off + (uint64_t)q->rle_cap * 4);
  q->off_rle_out = off; off = al256(off + (uint64_t)q->rle_cap * 4);
  q->off_run_start = off; off = al256(off + (uint64_t)q->rle_cap * 4);
  q->ws_per_block = off;
  q->arena_uni_cap = (uint32_t)std::min<uint64_t>(arena_ints, 0xFFFFFFF0ull);
  q->ring_stride = (uint32_t)ring_stride;
  q->threads = in.threads > 0 ? in.threads : (p.span == 1 ? 256 : 64);
  int64_t blocks = std::min<int64_t>(in.n_jobs_host, (int64_t)in.num_cus * (q->threads >= 512 ? 4 : q->threads >= 256 ? 8 : 16));
  blocks = std::min<int64_t>(blocks, (int64_t)(in.ws_limit / std::max<uint64_t>(q->ws_per_block, 1)));
  if (in.ws_budget > 0 && blocks > 1) blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)(in.ws_budget / std::max<uint64_t>(q->ws_per_block, 1))));
  if (blocks < 1) {
    const uint64_t fixed = q->ws_per_block - al256(arena_ints * 4);  // (what a workgroup needs beside its arena)
    if (in.ws_limit <= fixed + 4096) return refuse(q, why, TRGT_ERR_NOMEM, "wfa: workspace limit %llu B too small", (unsigned long long)in.ws_limit);
    return refuse(q, why, TRGT_ERR_NOMEM, "wfa: one workgroup needs %llu B of workspace, limit is %llu B", (unsigned long long)q->ws_per_block,
                  (unsigned long long)in.ws_limit);
  }
  q->blocks = blocks;
  // job counters | slot flags | 40 words of the lean kernels (3 x 8 statistics, their counters)
  q->counter_bytes = 16 + 4 * (uint64_t)blocks + 160;
  return TRGT_OK;
}

// which kernel the main launch runs, and its LDS
inline int plan_main(const WfaPlanIn& in, WfaPlan* q, const char** why) {
  const trgt_wfa_params& p = in.p;
  const wfa::Pen& pen = q->pen;
  const bool biwfa = p.memory_mode == 3;
  const int64_t mp = in.max_plen, mt = in.max_tlen, msum = in.max_sum;
  const int threads = q->threads;
  if (in.tag < 0 || in.tag > 3) return refuse(q, why, TRGT_ERR_INVALID, "wfa: no kernel tag %d", in.tag);
  const uint64_t seq_need = ((uint64_t)mp + 15) / 16 * 16 + (uint64_t)mt + 16;
  q->lds_seq_cap = (uint32_t)((std::min<uint64_t>(seq_need, 32 * 1024) + 15) & ~15ull);
  if (seq_need > 32 * 1024 || in.wfa_no_stage) q->lds_seq_cap = 0;  // too long: extend straight from global memory (L1/L2 cached)
  q->lds = q->lds_seq_cap;
  q->fast_dbg = in.skip_bt ? 1 : 0;
  if (p.metric == 3 && p.heuristic == 0 && !biwfa && q->lds_seq_cap > 0 && mt + q->score_bound < 65000 && threads % 64 == 0 && threads <= 256) {
    // LDS fast path (wfa_fast.hpp): ring of the live wavefronts as 16-bit offsets
    uint64_t wcap = ((uint64_t)msum + 8 + 7) & ~7ull;
    if (q->capped) {  // levels 0 .. max_score + 1: diagonals -(max_score + 1) .. text_begin_free + max_score + 1
      q->fast_koff = (uint32_t)(in.max_score + 4);
      wcap = std::min<uint64_t>(wcap, ((uint64_t)q->fast_koff + (uint64_t)p.text_begin_free + (uint64_t)in.max_score + 12 + 7) & ~7ull);
    }
    const uint64_t ring_bytes = (uint64_t)(std::max(pen.x, pen.o1 + pen.e1) + 1 + 2 * (pen.e1 + 1)) * wcap * 2;
    const uint64_t win_bytes = 4ull * (uint64_t)(mp + mt + 8);
    // (the byte copies of the two sequences are staged in the ring area, which is idle until level 0 is written)
    if (ring_bytes + win_bytes <= 96 * 1024 && (seq_need <= ring_bytes || q->capped)) {
      q->fast_wcap = (uint32_t)wcap; q->fast_ring_bytes = (uint32_t)((ring_bytes + 15) & ~15ull); q->lds = (uint64_t)q->fast_ring_bytes + win_bytes;
    }
  }
  // TRGT's flank-location configuration has instantiations of its own (wfa_fast.hpp, SPEC)
  const bool flank_pen = pen.x == 2 && pen.o1 == 5 && pen.e1 == 1 && p.span == 1 && p.pattern_begin_free == 0 && p.pattern_end_free == 0 && p.text_end_free < 0 && !in.no_spec;
  const bool fast_spec = flank_pen && q->fast_koff == 0 && p.text_begin_free < 0 && (threads == 256 || threads == 192);
  const bool win_spec = flank_pen && q->fast_koff != 0 && (in.tag == 2 || in.tag == 3) && threads == 64;  // the windowed launches of trgt_find_spans_batch
  // (TRGT_BAND_THREADS=256 / 128: the banded back-trace of what the pre-filter keeps with four / two waves per alignment -- its launch is as
  //  long as its slowest alignment, and a band of 2 s* + 2 s + 1 diagonals is several strips of a wave)
  const bool band_wide = flank_pen && q->fast_koff != 0 && in.tag == 3 && (threads == 256 || threads == 128);
  if (in.tag == 3 && !win_spec && !band_wide) return refuse(q, why, TRGT_ERR_INVALID, "wfa: the banded launch exists for the flank configuration only");
  if (q->fast_wcap > 0) {
    q->main = WFA_MAIN_FAST;
    q->main_id = band_wide ? (threads == 256 ? WFA_FAST_256_T3 : WFA_FAST_128_T3) : win_spec ? (in.tag == 3 ? WFA_FAST_64_T3 : WFA_FAST_64_T2)
                 : (fast_spec ? (threads == 192 ? WFA_FAST_192_T0 : WFA_FAST_256_T0) : WFA_FAST_ANY_T0) + in.tag;
  } else {  // the generic kernel keeps the descriptor rings of its three instances behind the staged sequences
    q->main = WFA_MAIN_GENERIC;
    q->main_id = wfa_generic_id(p.metric, threads == 64 && !in.wfa_no_wave_variant && (p.metric == 1 || p.metric == 3));
    q->ring_mask = wfa::RING - 1; q->ring_off = (q->lds_seq_cap + 15u) & ~15u;
    q->lds = (uint64_t)q->ring_off + 3 * wfa::RING * 5 * sizeof(wfa::WfDesc);
  }
  return TRGT_OK;
}

// the kernel in front of the generic one, for BiWFA batches of one wave per alignment
inline int plan_front(const WfaPlanIn& in, WfaPlan* q, const char** why) {
  const trgt_wfa_params& p = in.p;
  const wfa::Pen& pen = q->pen;
  q->jobs_bound = in.jobs_bound > 0 ? in.jobs_bound : in.n_jobs_host;  // (n_jobs_host may only bound the workgroups: the retry list holds every job)
  const bool one_wave_biwfa = p.memory_mode == 3 && p.span == 0 && q->threads == 64 && !in.has_ops && q->main == WFA_MAIN_GENERIC && !in.has_jobs2;
  if (one_wave_biwfa && !in.no_lean && (p.metric == 1 || (p.metric == 3 && pen.x == 2 && pen.o1 == 5 && pen.e1 == 1))) {
    // with a device-side job count the retry list must hold every job the lean kernels may hand on -- n_jobs_host only bounds the
    // workgroups then -- so the caller has to say how many there can be; a list that is too short would drop alignments
    if (in.has_n_jobs_dev && in.jobs_bound <= 0)
      return refuse(q, why, TRGT_ERR_INVALID, "wfa: a launch with a device-side job count needs jobs_bound (the capacity of the hand-over lists)");
    q->front = WFA_FRONT_LEAN;
  } else if (one_wave_biwfa && (p.metric == 1 || p.metric == 3) && !in.no_lds_wfa) {
    // dynamic LDS of a workgroup: sequences | two run-length buffers | descriptor rings (as many levels as the score scope needs) | the
    // region of the wavefronts.  Defaults sized for 12 workgroups per CU (one wave each; the registers allow no more): this kernel is all
    // latency, and the alignments that do not fit are few and go to the HBM variant.
    q->front = WFA_FRONT_ARENA;
    q->arena_id = wfa_arena_id(p.metric, !in.wfa_no_wave_variant);
    const uint32_t seq_cap = (uint32_t)std::max(256, in.lds_wfa_seq), rle_cap = 96, region = (uint32_t)std::max(2, in.lds_wfa_kb) * 1024u;
    uint32_t ring_levels = 2;
    while ((int)ring_levels < pen.scope) ring_levels *= 2;
    q->la_seq_cap = seq_cap; q->la_rle_cap = rle_cap; q->la_rle_tmp = seq_cap; q->la_rle_out = seq_cap + 4 * rle_cap;
    q->la_ring_off = seq_cap + 8 * rle_cap; q->la_ring_mask = ring_levels - 1;
    q->la_region = q->la_ring_off + 3 * ring_levels * 5 * (uint32_t)sizeof(wfa::WfDesc); q->la_region_bytes = region;
    q->la_gdesc_slots = std::min<uint32_t>(40, (region / 3) / (5 * (uint32_t)sizeof(wfa::WfDesc)));
    q->la_lds = (uint64_t)q->la_region + region;
  }
  return TRGT_OK;
}
}  // namespace wfa_plan_detail

// TRGT_OK and the plan, or the TRGT_ERR_* code of a launch that cannot be made with *why = its message (kept in the plan)
inline int wfa_plan(const WfaPlanIn& in, WfaPlan* q, const char** why) {
  using namespace wfa_plan_detail;
  *q = WfaPlan();
  int rc;
  if ((rc = plan_penalties(in.p, q, why)) || (rc = plan_workspace(in, q, why)) || (rc = plan_main(in, q, why)) || (rc = plan_front(in, q, why))) return rc;
  return TRGT_OK;
}

}  // namespace trgt
