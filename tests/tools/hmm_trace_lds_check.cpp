// tests/tools/hmm_trace_lds_check.cpp -- the LDS of a job of hmm_trace_ppl_kernel<G> (trgt_amd/csrc/hmm_trace_ppl_lds.hpp) held to its
// invariants on a host compiler, no GPU and no HIP:
//   g++ -std=c++17 -I trgt_amd/csrc tests/tools/hmm_trace_lds_check.cpp -o hmm_trace_lds_check && ./hmm_trace_lds_check
// For G = 8, 16 and every model of launch class 0 and beyond it up to the header's limits (S states, nb blocks):
//   every piece starts on a 16-byte boundary, no two pieces overlap, each is as large as what the kernel puts there,
//   a job's own carve-up fits the slot of any class it can belong to (larger S, larger nb), and the 64 / G slots of a wave fit 64 KB.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "hmm_trace_ppl_lds.hpp"

static int failures = 0;
#define HOLD(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a compile-time use: the launcher and the kernel call the same constexpr function
static_assert(hmm_trace_ppl_lds(8, HMM_TP_MAX_STATES, HMM_TP_MAX_BLOCKS).total * 8 <= 64 * 1024, "eight jobs of the largest class-0 model");
static_assert(hmm_trace_ppl_lds(16, HMM_TP_MAX_STATES, HMM_TP_MAX_BLOCKS).total * 4 <= 64 * 1024, "four jobs of the largest class-0 model");

int main() {
  for (int G : {8, 16}) {
    for (int S = 8; S <= HMM_TP_MAX_STATES; ++S) {
      for (int nb = 1; nb <= HMM_TP_MAX_BLOCKS; ++nb) {
        const HmmTracePplLds l = hmm_trace_ppl_lds(G, S, nb);
        // (offset, bytes the kernel uses there)
        const int mot_bytes = std::max(0, (S - 7 - (nb - 1)) / 3);
        const std::vector<std::pair<int, int>> pieces = {
            {l.tb, 12 * 4}, {l.inst, 16 * S}, {l.info, 4 * S}, {l.blocks, 16 * nb}, {l.flags, S}, {l.mot, mot_bytes}, {l.cnt, 4 * (nb - 1)},
            {l.rec, 8 * G}, {l.vis, 12 * HMM_TP_VIS}, {l.seq, HMM_TP_COLS + 1 + HMM_TP_CODE_PAD}, {l.stage, ((HMM_TP_COLS + 1) * G + 15) / 16 * 16}};  // (a chunk: up to HMM_TP_COLS + 1 rows, copied in 16-byte pieces)
        int end_before = 0;
        for (size_t i = 0; i < pieces.size(); ++i) {
          HOLD(pieces[i].first % 16 == 0, "G=%d S=%d nb=%d piece %zu at %d", G, S, nb, i, pieces[i].first);
          HOLD(pieces[i].first >= end_before, "G=%d S=%d nb=%d piece %zu at %d overlaps the one before (ends at %d)", G, S, nb, i, pieces[i].first, end_before);
          end_before = pieces[i].first + pieces[i].second;
        }
        HOLD(end_before <= l.total && l.total % 16 == 0, "G=%d S=%d nb=%d total %d", G, S, nb, l.total);
        // the staging window afterwards takes chunks of visits: whole records only
        HOLD(hmm_trace_ppl_stage_bytes(G) / 12 >= 1 && hmm_trace_ppl_stage_bytes(G) % 16 == 0, "G=%d stage %d", G, hmm_trace_ppl_stage_bytes(G));
        // a job's own carve-up inside the slot of a class with larger models
        if (S < HMM_TP_MAX_STATES) HOLD(hmm_trace_ppl_lds(G, S + 1, nb).total >= l.total, "G=%d S=%d nb=%d not monotone in S", G, S, nb);
        if (nb < HMM_TP_MAX_BLOCKS) HOLD(hmm_trace_ppl_lds(G, S, nb + 1).total >= l.total, "G=%d S=%d nb=%d not monotone in nb", G, S, nb);
        HOLD((64 / G) * l.total <= 64 * 1024, "G=%d S=%d nb=%d: %d jobs x %d B", G, S, nb, 64 / G, l.total);
      }
    }
    const HmmTracePplLds top = hmm_trace_ppl_lds(G, HMM_TP_MAX_STATES, HMM_TP_MAX_BLOCKS), str3 = hmm_trace_ppl_lds(G, 17, 2);
    std::printf("lds G=%d largest_job=%d wave=%d str3_job=%d\n", G, top.total, (64 / G) * top.total, str3.total);
  }
  if (failures) { std::printf("hmm_trace_lds_check: %d FAILED\n", failures); return 1; }
  std::printf("hmm_trace_lds_check: all held\n");
  return 0;
}
