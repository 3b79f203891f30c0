// trgt_amd/csrc/hmm_trace_ppl_lds.hpp -- the LDS of one job of hmm_trace_ppl_kernel<G> (hmm_trace_ppl.hpp), shared by the kernel and its
// launcher (hmm_batch.hpp).  No HIP here: tests/tools/hmm_trace_lds_check.cpp compiles it with the host compiler and holds it to its
// invariants (pieces of 16-byte multiples that do not overlap, the 64 / G jobs of a wave inside 64 KB).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HMM_TP_HD __host__ __device__
#else
#define HMM_TP_HD
#endif

constexpr int HMM_TP_COLS = 64;      // back-pointer columns staged per chunk (rows of G bytes: 528 / 1 056 bytes with the two spare columns)
constexpr int HMM_TP_VIS = 32;       // motif visits kept in LDS; the others go to the job's workspace (hmm_decode_visits reads them back in chunks)
constexpr int HMM_TP_CODE_PAD = 16;  // symbol codes behind the staged columns (HMM_CODE_PAD: the bases of a motif copy that starts in the last of them)
constexpr int HMM_TP_MAX_STATES = 32, HMM_TP_MAX_BLOCKS = 8;  // launch class 0: at most 32 states, hence at most 6 motifs (7 blocks) of 8 bases in all

// Offsets of the pieces inside a job's slot, and the slot's size.  Only what the trace-back reads: nothing of the fill's (score columns,
// transition and emission terms, the per-state block and back-pointer columns).
struct HmmTracePplLds {
  int tb;      // the walk's state: the words TB_* (hmm_traceback.hpp)
  int inst;    // [S][4] hmm_pred_entry
  int info;    // [S] the trace-back word of a state
  int blocks;  // [4][nb]
  int flags;   // [S]
  int mot;     // motif bytes
  int cnt;     // [n_motifs]
  int rec;     // [G][2] (state, column) of the steps of a round
  int vis;     // [HMM_TP_VIS][3] the first motif visits
  int seq;     // symbol codes of the staged columns (+ HMM_TP_CODE_PAD)
  int stage;   // staged back-pointer columns; afterwards the chunks of overflowed visits
  int total;
};
HMM_TP_HD constexpr int hmm_tp_up16(int v) { return (v + 15) & ~15; }
HMM_TP_HD constexpr int hmm_trace_ppl_stage_bytes(int G) { return (HMM_TP_COLS + 2) * G; }  // (a chunk starts on an even column: one more than HMM_TP_COLS, and one to spare)
// G: lanes per job (8 / 16); S, nb: states and blocks of the model -- the job's own for the carve-up, the largest of the class for the
// slot's size (every piece grows with S and nb, so a job's own pieces fit the class's slot).
HMM_TP_HD constexpr HmmTracePplLds hmm_trace_ppl_lds(int G, int S, int nb) {
  HmmTracePplLds l{};
  int o = 0;
  l.tb = o; o += 64;
  l.inst = o; o += 16 * S;
  l.info = o; o += hmm_tp_up16(4 * S);
  l.blocks = o; o += 16 * nb;
  l.flags = o; o += hmm_tp_up16(S);
  l.mot = o; o += hmm_tp_up16(S > 7 ? (S - 7) / 3 : 1);
  l.cnt = o; o += hmm_tp_up16(4 * nb);
  l.rec = o; o += 8 * G;
  l.vis = o; o += 12 * HMM_TP_VIS;
  l.seq = o; o += hmm_tp_up16(HMM_TP_COLS + 2 + HMM_TP_CODE_PAD);
  l.stage = o; o += hmm_tp_up16(hmm_trace_ppl_stage_bytes(G));
  l.total = o;
  return l;
}
