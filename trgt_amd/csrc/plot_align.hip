// trgt_amd/csrc/plot_align.hip -- trgt_plot_align_batch: the alignments `trgt plot` draws, for a batch of panels (include/trgt_hip_plot.h).
//
// Reference (PacificBiosciences/trgt v3.0.0, src/trvz/):
//   get_allele_align  align_allele.rs:7-14      mode 0: align_consensus, then align_reads
//   align_consensus   align_consensus.rs:9-31   flank segments around align_motifs of the allele
//   align_motifs      align_consensus.rs:35-122 Hmm::label, remove_imperfect_motifs(.., 6), label_motifs, get_events -> typed segments
//   align_reads       align_reads.rs:7-28       one end-to-end alignment per read, convert (:31-113), project_betas, the sort of :26
//   project_betas     read.rs:24-66
//   align (waterfall) waterfall_plot.rs:42-123  mode 1: two flank alignments, align_motifs of the read's repeat part, the padding
//                                               segment, the three-part split of the betas; convert :134-191; the sort of :28-37
//
// This unit is a CALLER of hmm_batch_impl and wfa_batch_impl, like locus.hip: the state paths and the run-length CIGARs stay in HBM and
// two kernels of this file turn them into segments.  Both run one wave per item, four items per 256-thread block (as locus_meth.hip).
//   plot_motif_segs_kernel  one wave per HMM job (mode 0: a panel's consensus, mode 1: a read): align_motifs over the state path, 64
//                           path entries per step, in four passes -- (1) per motif visit, at its block end, whether
//                           remove_imperfect_motifs drops it: the visit's type goes to its first base; (2) every base takes the type
//                           of its visit: motif_by_base; (3) events, run starts by ballot, widths by popcount, compacted stores;
//                           (4) mode 0: seg_type_by_ref of convert, run-length encoded, for the second kernel.
//   plot_read_segs_kernel   one wave per read: convert and project_betas over the run-length CIGAR, 64 runs per step.
// Order of a call: checks, one upload, hmm_batch_impl, plot_motif_segs_kernel, wfa_batch_impl (on_device), plot_read_segs_kernel,
// copy-out.  One stream.
#include "common.hpp"
#include "hmm_host.hpp"
#include "wfa_host.hpp"

#include <algorithm>
#include <climits>
#include <numeric>

namespace trgt {
namespace plot {

constexpr uint32_t SEG_LF = 0xFFFEu, SEG_RF = 0xFFFFu;
constexpr uint32_t OP_MATCH = 0, OP_SUBST = 1, OP_INS = 2, OP_DEL = 3;   // AlignOp, trvz/align.rs:18-24
constexpr int RUNS_LDS = 512;   // seg-type runs of a panel a wave of plot_read_segs_kernel keeps in LDS (else it reads them from HBM)

struct MotifItem {     // one wave of plot_motif_segs_kernel
  uint64_t seq_off;    // the repeat's bases in the call's slab
  uint64_t path_off;   // its state path (u16 entries)
  uint64_t tbb_off;    // motif_by_base (u16 entries of the workspace)
  uint64_t seg_off;    // where its segments go: mode 0 the panel's slot of pseg (segment 0: the left flank), mode 1 workspace
  uint64_t run_off;    // mode 0: the panel's seg-type runs (pairs of the workspace)
  uint32_t seq_len, path_cap, set;
  int32_t hjob;        // index into the HMM batch's per-job results; -1: an empty repeat, no job
  uint32_t lf, rf;
};
struct ReadItem {      // one wave of plot_read_segs_kernel
  uint64_t rseg_off;   // the read's slot (segments)
  uint64_t beta_off;   // first beta of the read
  uint64_t tr_seg_off; // mode 1: the segments of its repeat part in the workspace
  uint64_t run_off;    // mode 0: the panel's seg-type runs
  uint32_t n_beta, nb_lf, nb_tr;   // betas of the read; mode 1: those in front of lf, in front of lf + tr
  uint32_t read_len, ref_len, cap;
  int32_t job[2];      // alignment jobs: mode 0 {read vs consensus, -1}; mode 1 {left flank, right flank}, -1: an empty flank
  uint32_t item;       // mode 0: the panel's MotifItem (n_runs); mode 1: the read's own (n_tr)
  uint32_t lf, tr, pad_w;          // mode 1: left flank, repeat part, longest_read - read_len
  uint32_t pad;
};

struct MotifArgs {
  const MotifItem* items; uint32_t n_items; int mode;
  const uint8_t* slab; const uint16_t* path; const uint32_t* path_len;
  const HmmSetDev* sets; const uint8_t* model;
  uint16_t* tbb; uint32_t* work_seg; uint32_t* runs; uint32_t* n_tr; uint32_t* n_runs;
  uint32_t* pseg; uint32_t* n_pseg;
};
struct ReadArgs {
  const ReadItem* items; uint32_t n_items; int mode;
  const JobDev* jobs; const uint32_t* cigar; const uint32_t* cigar_len; const int32_t* status; const int32_t* wfa_score;
  const uint32_t* runs; const uint32_t* n_runs; const uint32_t* work_seg; const uint32_t* n_tr;
  const uint32_t* beta_pos; int32_t* beta_proj;
  uint32_t* rseg; uint32_t* n_rseg; int32_t* score; unsigned int* flag;
};

__device__ inline int popc64(uint64_t v) { return __popcll((unsigned long long)v); }
__device__ inline int top_bit(uint64_t v) { return 63 - (int)__builtin_clzll((unsigned long long)v); }   // v != 0
__device__ inline uint32_t rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }   // lane is wave-uniform

// The trace-back word of a state, laid out as hmm_state_info (hmm_traceback.hpp) lays it out: kind (0 outside any block, 1 block
// start, 2 block end, 3 skip state, 4 match, 5 insertion, 6 deletion) | block << 8 | expected motif base << 16 (match states)
__device__ inline uint32_t state_word(const int st, const int S, const int nb, const int16_t* __restrict__ block_of, const uint32_t* __restrict__ blocks,
                                      const uint8_t* __restrict__ motif_bytes) {
  if (st < 0 || st >= S) return 0u;
  const int blk = block_of[st];
  if (blk < 0 || blk >= nb) return 0u;
  uint32_t kind, expected = 0;
  const int bstart = (int)blocks[0 * nb + blk], bend = (int)blocks[1 * nb + blk];
  if (st == bstart) kind = 1;
  else if (st == bend) kind = 2;
  else if (blk == nb - 1) kind = 3;
  else {
    const int mlen = (int)blocks[2 * nb + blk], off = st - bstart - 1, k = off / mlen;
    kind = 4u + (uint32_t)k;
    if (k == 0) expected = motif_bytes[blocks[3 * nb + blk] + off];
  }
  return kind | ((uint32_t)(blk & 0xFF) << 8) | (expected << 16);
}

// One step of a pass over the state path: 64 entries, one per lane
struct PathStep {
  int st, kind, blk, expected;
  bool valid, emits;
  uint32_t bp;       // bases in front of the entry: the position of the base it emits, or of the next base
  uint64_t em, starts;
};
__device__ inline PathStep path_step(const uint16_t* __restrict__ path, const uint32_t n, const uint32_t base, const int lane, const uint32_t bases_before,
                                     const int S, const int nb, const int16_t* block_of, const uint32_t* blocks, const uint8_t* motif_bytes) {
  PathStep p;
  const uint32_t j = base + (uint32_t)lane;
  p.valid = j < n;
  p.st = p.valid ? (int)path[j] : 0;
  const uint32_t w = p.valid ? state_word(p.st, S, nb, block_of, blocks, motif_bytes) : 0u;
  p.kind = (int)(w & 7u); p.blk = (int)((w >> 8) & 0xFFu); p.expected = (int)((w >> 16) & 0xFFu);
  p.emits = p.kind == 3 || p.kind == 4 || p.kind == 5;
  p.em = __ballot(p.emits);
  p.starts = __ballot(p.kind == 1);
  p.bp = bases_before + (uint32_t)popc64(p.em & (((uint64_t)1 << lane) - 1));
  return p;
}
// The value the entry's visit holds: start lanes carry `at_start`; the other lanes take it from the last start lane in front of them, or
// from the steps before (carry, which is advanced to the step's last start).
__device__ inline uint32_t visit_value(const PathStep& p, const int lane, const uint32_t at_start, uint32_t& carry) {
  const uint64_t sb = p.starts & ((((uint64_t)1 << lane) - 1) | ((uint64_t)1 << lane));
  const int src = sb ? top_bit(sb) : lane;
  const uint32_t v = (uint32_t)__shfl((int)at_start, src);
  const uint32_t mine = sb ? v : carry;
  if (p.starts) carry = rl(at_start, top_bit(p.starts));
  return mine;
}

__global__ void __launch_bounds__(256) plot_motif_segs_kernel(const MotifArgs a) {
  const uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (item >= a.n_items) return;
  const int lane = (int)(threadIdx.x & 63u);
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const MotifItem it = a.items[item];
  const uint32_t L = it.seq_len;
  uint32_t* const seg = (a.mode == 0 ? a.pseg : a.work_seg) + 2 * (it.seg_off + (a.mode == 0 ? 1u : 0u));   // (mode 0: behind the left-flank segment)
  const uint32_t seg_cap = 2u * L + 1u;
  uint32_t* const runs = a.runs + 2 * it.run_off;
  uint32_t n_out = 0;

  if (it.hjob >= 0 && L > 0) {
    const HmmSetDev sd = a.sets[it.set];
    const int S = (int)sd.S, nb = (int)sd.n_blocks;
    const int16_t* block_of = reinterpret_cast<const int16_t*>(a.model + sd.off_block);
    const uint32_t* blocks = reinterpret_cast<const uint32_t*>(a.model + sd.off_blocks);
    const uint8_t* motif_bytes = a.model + sd.off_motifs;
    const uint16_t* path = a.path + it.path_off;
    const uint32_t n = min(a.path_len[it.hjob], it.path_cap);
    const uint8_t* seq = a.slab + it.seq_off;
    uint16_t* tbb = a.tbb + it.tbb_off;
    const uint32_t skip_type = (uint32_t)(nb - 1);

    // ---- pass 1: remove_imperfect_motifs(.., 6) (operations.rs:6-80), decided at every block end: the visit's bases are
    // [first, bp); a copy of a motif of at most 6 bases is dropped when it is shorter than the motif or its first bases differ from it
    uint32_t bases = 0, first_carry = 0;
    for (uint32_t base = 0; base < n; base += 64) {
      const PathStep p = path_step(path, n, base, lane, bases, S, nb, block_of, blocks, motif_bytes);
      const uint32_t first = visit_value(p, lane, p.bp, first_carry);
      if (p.kind == 2 && p.bp > first && first < L) {
        uint32_t type = (uint32_t)p.blk;
        const uint32_t mlen = blocks[2 * nb + p.blk];
        if (p.blk != nb - 1 && mlen <= 6u) {
          bool drop = p.bp - first < mlen;
          if (!drop) {
            const uint8_t* mot = motif_bytes + blocks[3 * nb + p.blk];
            for (uint32_t i = 0; i < mlen; ++i) drop |= mot[i] != 'N' && seq[first + i] != mot[i];
          }
          if (drop) type = skip_type;
        }
        tbb[first] = (uint16_t)type;
      }
      bases += (uint32_t)popc64(p.em);
    }
    __threadfence_block();
    // ---- pass 2: motif_by_base (align_consensus.rs:43-47): every base takes the type of its visit
    bases = 0;
    uint32_t type_carry = skip_type;
    for (uint32_t base = 0; base < n; base += 64) {
      const PathStep p = path_step(path, n, base, lane, bases, S, nb, block_of, blocks, motif_bytes);
      const uint32_t at_start = p.kind == 1 ? (uint32_t)tbb[min(p.bp, L - 1)] : 0u;
      const uint32_t type = visit_value(p, lane, at_start, type_carry);
      if (p.emits && p.bp < L) tbb[p.bp] = (uint16_t)type;
      bases += (uint32_t)popc64(p.em);
    }
    __threadfence_block();
    // ---- pass 3: get_events (events.rs:17-86) and the loop of align_consensus.rs:54-104 with its final merge (:108-119).  An entry
    // contributes (op, seg type, width 0 or 1); the type is motif_by_base at the entry's base position, at the end of the sequence
    // that of the last base.  MotifStart / MotifEnd / Trans contribute nothing, and the merge joins what they separated: a run is a
    // maximal stretch of contributing entries with one (op, seg type).
    bases = 0; type_carry = skip_type;
    bool have_open = false;
    uint32_t open_key = 0xFFFFFFFFu, open_w = 0;
    for (uint32_t base = 0; base < n; base += 64) {
      const PathStep p = path_step(path, n, base, lane, bases, S, nb, block_of, blocks, motif_bytes);
      const uint32_t j = base + (uint32_t)lane;
      const uint32_t here = (uint32_t)tbb[min(p.bp, L - 1)];   // motif_by_base[base_pos], or the last base's
      const uint32_t own = visit_value(p, lane, p.kind == 1 ? here : 0u, type_carry);   // the type of the entry's own visit
      const bool dropped = p.kind != 0 && p.blk != nb - 1 && own == skip_type;          // its visit became skip states
      bool prod = false; uint32_t op = OP_MATCH, w = 1;
      if (p.kind == 3) prod = true;                                                     // Skip
      else if (p.kind == 4) {                                                           // Match / Mismatch (a dropped copy: Skip)
        prod = true;
        const int q = p.bp < L ? (int)seq[p.bp] : 0;
        op = dropped || q == p.expected || p.expected == 'N' ? OP_MATCH : OP_SUBST;
      } else if (p.kind == 5) { prod = true; op = dropped ? OP_MATCH : OP_DEL; }        // Ins -> AlignOp::Del
      else if (p.kind == 6) { prod = !dropped; op = OP_INS; w = 0; }                    // Del -> a width-0 AlignOp::Ins
      else if (p.kind == 1) {                                                           // MotifStart: path[j + 1] - s - 1 implied Del events
        const int nxt = j + 1 < n ? (int)path[j + 1] : p.st + 1;
        prod = !dropped && nxt - p.st - 1 > 0; op = OP_INS; w = 0;
      }
      const uint32_t key = op | (here << 8);
      const uint64_t P = __ballot(prod), pb = P & below;
      const uint32_t before = (uint32_t)__shfl((int)key, pb ? top_bit(pb) : lane);
      const bool run_start = prod && key != (pb ? before : open_key);
      const uint64_t R = __ballot(run_start), W = __ballot(prod && w != 0);
      const int first_rs = R ? __ffsll((unsigned long long)R) - 1 : 64;
      open_w += (uint32_t)popc64(first_rs == 64 ? W : W & (((uint64_t)1 << first_rs) - 1));
      if (R) {
        if (have_open) { if (lane == 0 && n_out < seg_cap) { seg[2 * n_out] = open_w; seg[2 * n_out + 1] = open_key; } ++n_out; }
        const uint64_t later = lane == 63 ? 0ull : R & ~((((uint64_t)1 << lane) - 1) | ((uint64_t)1 << lane));
        const int end = later ? __ffsll((unsigned long long)later) - 1 : 64;
        const uint64_t span = (end == 64 ? ~0ull : (((uint64_t)1 << end) - 1)) & ~below;
        const uint32_t width = (uint32_t)popc64(W & span);
        const uint32_t at = n_out + (uint32_t)popc64(R & below);
        if (run_start && later && at < seg_cap) { seg[2 * at] = width; seg[2 * at + 1] = key; }
        const int last = top_bit(R);
        open_key = rl(key, last); open_w = rl(width, last); have_open = true;
        n_out += (uint32_t)popc64(R) - 1u;
      }
      bases += (uint32_t)popc64(p.em);
    }
    if (have_open) { if (lane == 0 && n_out < seg_cap) { seg[2 * n_out] = open_w; seg[2 * n_out + 1] = open_key; } ++n_out; }
    n_out = min(n_out, seg_cap);
  }
  if (lane == 0) a.n_tr[item] = n_out;
  if (a.mode != 0) return;

  // ---- mode 0: the flank segments of align_consensus (:10-14, :25-29), and seg_type_by_ref of convert (align_reads.rs:35-42) run-length
  // encoded: (first reference position, seg type) per run.  A base of the repeat is one reference position of its type whatever the op
  // of its segment, Ins segments hold none: the runs are those of motif_by_base, between the two flanks.
  uint32_t* const ps = a.pseg + 2 * it.seg_off;
  if (lane == 0) {
    ps[0] = it.lf; ps[1] = OP_MATCH | (SEG_LF << 8);
    ps[2 * (n_out + 1)] = it.rf; ps[2 * (n_out + 1) + 1] = OP_MATCH | (SEG_RF << 8);
    a.n_pseg[item] = n_out + 2;
  }
  uint32_t nr = 0;
  if (it.lf > 0) { if (lane == 0) { runs[0] = 0; runs[1] = SEG_LF; } nr = 1; }
  if (it.hjob >= 0 && L > 0) {
    const uint16_t* tbb = a.tbb + it.tbb_off;
    for (uint32_t base = 0; base < L; base += 64) {
      const uint32_t b = base + (uint32_t)lane;
      const bool v = b < L;
      const uint32_t t = v ? (uint32_t)tbb[b] : 0u, tp = v && b > 0 ? (uint32_t)tbb[b - 1] : 0xFFFFFFFFu;
      const bool rs = v && t != tp;
      const uint64_t R = __ballot(rs);
      const uint32_t at = nr + (uint32_t)popc64(R & below);
      if (rs && at < L + 2) { runs[2 * at] = it.lf + b; runs[2 * at + 1] = t; }
      nr += (uint32_t)popc64(R);
    }
  }
  if (it.rf > 0) { if (lane == 0 && nr < L + 2) { runs[2 * nr] = it.lf + L; runs[2 * nr + 1] = SEG_RF; } ++nr; }
  if (lane == 0) a.n_runs[item] = min(nr, L + 2);
}

// ---- convert and project_betas over a run-length CIGAR

// inclusive scan over the wave
__device__ inline uint32_t wave_scan(uint32_t v, const int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)v, o); if (lane >= o) v += u; }
  return v;
}
// the panel's seg-type runs: in LDS when they fit
struct Runs {
  const uint32_t* g; const uint32_t* l; uint32_t n; bool in_lds;
  __device__ inline uint32_t start(uint32_t k) const { return in_lds ? l[2 * k] : g[2 * k]; }
  __device__ inline uint32_t type(uint32_t k) const { return in_lds ? l[2 * k + 1] : g[2 * k + 1]; }
  __device__ inline uint32_t find(uint32_t x) const {   // the last run that starts at or in front of x (n > 0, the first run starts at 0)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (start(mid) <= x) lo = mid; else hi = mid; }
    return lo;
  }
};

// One alignment: its segments go to seg[seg_at ..] (at most cap in all; returns the new count), its betas -- bpos[0 .. nbeta), read positions
// less p_sub in the alignment's text -- to bproj, plus p_add.  CUT: the runs are cut at the seg-type boundaries of the consensus (mode 0);
// else every segment has const_type.
template <bool CUT>
__device__ inline uint32_t convert_cigar(const int lane, const uint32_t* __restrict__ cig, const uint32_t clen, const Runs& rv, const uint32_t const_type, const uint32_t ref_len,
                                         uint32_t* __restrict__ seg, uint32_t seg_at, const uint32_t cap, const uint32_t* __restrict__ bpos, int32_t* __restrict__ bproj,
                                         const uint32_t nbeta, const uint32_t p_sub, const uint32_t p_add) {
  uint32_t ref_before = 0, read_before = 0, beta_at = 0, prev_op = OP_MATCH;
  for (uint32_t base = 0; base < clen; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    const bool v = i < clen;
    const uint32_t e = v ? cig[i] : 0u, len = e >> 4, code = e & 15u;
    // cigar_get_CIGAR(show_mismatches = true): 7 '=', 8 'X', 1 'I', 2 'D' (WfaOp Match / Subst / Ins / Del)
    const uint32_t op = code == 8u ? OP_SUBST : code == 1u ? OP_INS : code == 2u ? OP_DEL : OP_MATCH;
    const uint32_t ra = v && op != OP_INS ? len : 0u, sa = v && op != OP_DEL ? len : 0u;
    const uint32_t r1 = ref_before + wave_scan(ra, lane), s1 = read_before + wave_scan(sa, lane);
    const uint32_t r0 = r1 - ra, s0 = s1 - sa;
    // ---- convert: align_reads.rs:31-113 (CUT), waterfall_plot.rs:134-191
    uint32_t k0 = 0, pieces = v ? 1u : 0u;
    if (CUT && v && rv.n > 0) {
      // an insertion takes the type of the next reference base, a trailing one that of the last base (:47-53)
      if (op == OP_INS || len == 0) k0 = rv.find(min(r0, ref_len - 1));
      else { k0 = rv.find(r0); pieces = rv.find(r0 + len - 1) - k0 + 1; }
    }
    const uint32_t p1 = wave_scan(pieces, lane), at0 = seg_at + p1 - pieces;
    for (uint32_t q = 0; q < pieces; ++q) {
      uint32_t width = op == OP_INS ? 0u : len, type = const_type;
      if (CUT && rv.n > 0) {
        type = rv.type(k0 + q);
        if (op != OP_INS && len != 0) {
          const uint32_t lo = max(r0, rv.start(k0 + q)), hi = k0 + q + 1 < rv.n ? min(r0 + len, rv.start(k0 + q + 1)) : r0 + len;
          width = hi - lo;
        }
      }
      if (at0 + q < cap) { seg[2 * (at0 + q)] = width; seg[2 * (at0 + q) + 1] = op | (type << 8); }
    }
    seg_at += rl(p1, 63);
    // ---- project_betas (read.rs:24-66) over run-length input, one lane per beta.  The betas of this step are those at read positions
    // [step_lo, step_hi): sorted, so they follow the ones placed so far.  A beta at p lies in the last run of the step that starts at
    // or in front of p -- a deletion starts where the next read-consuming run does, so that run is never a deletion unless p is
    // behind the step.  It is dropped inside an insertion, and at the run's first base when the run in front is a deletion: the
    // reference's loop consumes the beta at the first deletion operation, where at_pos holds and is_visible does not.
    const uint32_t step_lo = read_before, step_hi = rl(s1, 63);
    const uint32_t s0_key = v ? s0 : 0xFFFFFFFFu;
    if (bproj) {
      while (beta_at < nbeta) {   // (wave-uniform)
        const uint32_t bi = beta_at + (uint32_t)lane;
        const bool bv = bi < nbeta;
        const uint32_t p = bv ? bpos[bi] - p_sub : 0xFFFFFFFFu;
        const bool mine = bv && p >= step_lo && p < step_hi;
        uint32_t lo = 0;
#pragma unroll
        for (int stp = 32; stp >= 1; stp >>= 1) {
          const uint32_t cand = lo + (uint32_t)stp;
          const uint32_t sv = (uint32_t)__shfl((int)s0_key, (int)(cand & 63u));
          if (cand < 64u && sv <= p) lo = cand;
        }
        const uint32_t run_op = (uint32_t)__shfl((int)op, (int)lo), run_s0 = (uint32_t)__shfl((int)s0, (int)lo), run_r0 = (uint32_t)__shfl((int)r0, (int)lo);
        const uint32_t op_before = (uint32_t)__shfl((int)op, (int)(lo > 0 ? lo - 1 : 0));
        const uint32_t front = lo > 0 ? op_before : prev_op;
        if (mine) {
          const bool drop = run_op == OP_INS || run_op == OP_DEL || (p == run_s0 && front == OP_DEL);
          bproj[bi] = drop ? -1 : (int32_t)(run_r0 + (p - run_s0) + p_add);
        }
        const uint64_t m = __ballot(mine), beyond = __ballot(bv && p >= step_hi);
        beta_at += (uint32_t)popc64(m);
        if (beyond || !m) break;   // the rest belongs to later steps (or: nothing of this chunk was placed here)
      }
    }
    const uint32_t n_here = min(64u, clen - base);
    prev_op = rl(op, (int)n_here - 1);
    ref_before = rl(r1, 63); read_before = step_hi;
  }
  return seg_at;
}

__global__ void __launch_bounds__(256) plot_read_segs_kernel(const ReadArgs a) {
  __shared__ uint32_t l_runs[4][2 * RUNS_LDS];
  const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= a.n_items) return;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const ReadItem it = a.items[r];
  uint32_t* const seg = a.rseg + 2 * it.rseg_off;
  int32_t* const bproj = a.beta_proj ? a.beta_proj + it.beta_off : nullptr;
  const uint32_t* const bpos = a.beta_pos + it.beta_off;
  // betas the alignments never reach stay -1
  if (bproj) for (uint32_t i = (uint32_t)lane; i < it.n_beta; i += 64) bproj[i] = -1;
  bool bad = false;
  for (int k = 0; k < 2; ++k) if (it.job[k] >= 0 && a.status[it.job[k]] != TRGT_WF_COMPLETED) bad = true;
  if (bad) {
    if (lane == 0) { a.n_rseg[r] = 0; if (a.score) a.score[r] = INT_MIN; atomicMin(a.flag, r); }
    return;
  }
  uint32_t n = 0;
  Runs rv{nullptr, nullptr, 0, false};
  if (a.mode == 0) {
    rv.g = a.runs + 2 * it.run_off; rv.n = a.n_runs[it.item];
    if (rv.n <= (uint32_t)RUNS_LDS) {
      for (uint32_t i = (uint32_t)lane; i < 2 * rv.n; i += 64) l_runs[wave][i] = rv.g[i];
      rv.l = l_runs[wave]; rv.in_lds = true;
      __threadfence_block();
    }
    const JobDev jd = a.jobs[it.job[0]];
    const uint32_t clen = min(a.cigar_len[it.job[0]], jd.pat_len + jd.txt_len + 1u);
    n = convert_cigar<true>(lane, a.cigar + jd.cigar_off, clen, rv, 0u, it.ref_len, seg, 0u, it.cap, bpos, bproj, it.n_beta, 0u, 0u);
    if (lane == 0 && a.score) a.score[r] = a.wfa_score[it.job[0]];
  } else {
    // waterfall_plot.rs:42-123: the left flank's alignment, the repeat part's segments, the deletion that lines up the right flanks,
    // the right flank's alignment; betas in three parts (:74-115)
    if (it.job[0] >= 0) {
      const JobDev jd = a.jobs[it.job[0]];
      const uint32_t clen = min(a.cigar_len[it.job[0]], jd.pat_len + jd.txt_len + 1u);
      n = convert_cigar<false>(lane, a.cigar + jd.cigar_off, clen, rv, SEG_LF, it.lf, seg, n, it.cap, bpos, bproj, it.nb_lf, 0u, 0u);
    }
    const uint32_t ntr = a.n_tr[it.item];
    const uint32_t* src = a.work_seg + 2 * it.tr_seg_off;
    for (uint32_t i = (uint32_t)lane; i < 2 * ntr; i += 64) if (n + i / 2 < it.cap) seg[2 * n + i] = src[i];
    n += ntr;
    if (bproj) for (uint32_t i = it.nb_lf + (uint32_t)lane; i < it.nb_tr; i += 64) bproj[i] = (int32_t)bpos[i];
    if (it.pad_w > 0) { if (lane == 0 && n < it.cap) { seg[2 * n] = it.pad_w; seg[2 * n + 1] = OP_DEL | (SEG_RF << 8); } ++n; }
    if (it.job[1] >= 0) {
      const JobDev jd = a.jobs[it.job[1]];
      const uint32_t clen = min(a.cigar_len[it.job[1]], jd.pat_len + jd.txt_len + 1u);
      n = convert_cigar<false>(lane, a.cigar + jd.cigar_off, clen, rv, SEG_RF, it.read_len - it.lf - it.tr, seg, n, it.cap, bpos + it.nb_tr, bproj ? bproj + it.nb_tr : nullptr,
                               it.n_beta - it.nb_tr, it.lf + it.tr, it.lf + it.tr + it.pad_w);
    }
    if (lane == 0 && a.score) a.score[r] = INT_MIN;
  }
  if (lane == 0) a.n_rseg[r] = min(n, it.cap);
}

// Segments on their way to a host array: the used part of every slot, gathered into one dense buffer -- only the segments produced
// cross PCIe, not the slots of trgt_plot_seg_capacity (cf. cigar_pack_kernel, wfa.hip).  Item i's slot offset is the 8 bytes at
// items + i * stride + field.
__global__ void __launch_bounds__(256) plot_pack_segs_kernel(const uint32_t* __restrict__ seg, const uint8_t* __restrict__ items, uint32_t stride, uint32_t field, uint32_t n_items,
                                                             const uint32_t* __restrict__ n, const uint64_t* __restrict__ dst_off, uint32_t* __restrict__ packed) {
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n_items) return;
  const uint64_t slot = *reinterpret_cast<const uint64_t*>(items + (size_t)i * stride + field);
  const uint32_t* src = seg + 2 * slot;
  uint32_t* dst = packed + 2 * dst_off[i];
  for (uint32_t k = threadIdx.x & 63u; k < 2 * n[i]; k += 64) dst[k] = src[k];
}

static uint64_t seg_capacity(int32_t mode, uint32_t ref_len, uint32_t read_len) {
  if (mode == 0) return 2ull * ref_len + read_len + 3ull;
  return 2ull * std::max(ref_len, read_len) + 2ull;
}

// host view of the bytes [lo, hi) of a blob that may live on the device
static int host_view(trgt_hip_ctx* c, const uint8_t* blob, bool on_device, uint64_t lo, uint64_t hi, std::vector<uint8_t>& keep, const uint8_t** view) {
  if (!on_device || hi <= lo) { *view = blob; return TRGT_OK; }
  keep.resize((size_t)(hi - lo));
  TRGT_HIP_TRY(c, hipMemcpy(keep.data(), blob + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
  *view = keep.data() - lo;
  return TRGT_OK;
}
static inline bool is_acgt(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
// whether a byte of [p, p + n) lies outside ACGT, without a branch per byte: byte compares and an OR, which the compiler vectorises (a
// batch has megabytes of reads, and the byte-by-byte loop with its early exit was 1.5 of the call's 8 ms)
static inline bool any_not_acgt(const uint8_t* p, size_t n) {
  uint8_t bad = 0;
  for (size_t i = 0; i < n; ++i) bad |= (uint8_t)!((p[i] == 'A') | (p[i] == 'C') | (p[i] == 'G') | (p[i] == 'T'));
  return bad != 0;
}
static inline size_t first_not_acgt(const uint8_t* p, size_t n) {   // n: none
  if (!any_not_acgt(p, n)) return n;
  size_t i = 0;
  while (is_acgt(p[i])) ++i;
  return i;
}

}  // namespace plot
}  // namespace trgt

using namespace trgt;

extern "C" uint64_t trgt_plot_seg_capacity(int32_t mode, uint32_t ref_len, uint32_t read_len) { return plot::seg_capacity(mode, ref_len, read_len); }

extern "C" int trgt_plot_kernel_ms(const trgt_hip_ctx* c, double out[2]) {
  if (!c || !out) return TRGT_ERR_INVALID;
  out[0] = c->plot_ms[0]; out[1] = c->plot_ms[1];
  return TRGT_OK;
}

extern "C" int trgt_plot_align_batch(trgt_hip_ctx* c, const trgt_plot_in* in, trgt_plot_out* out) {
  if (!c) return TRGT_ERR_INVALID;
  if (!in || !out) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: null argument");
  const int mode = in->mode;
  if (mode != 0 && mode != 1) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: mode %d (0: allele plot, 1: waterfall)", mode);
  const int64_t np = in->n_panels;
  if (np < 0 || in->n_sets < 0) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: n_panels %lld, n_sets %d", (long long)np, in->n_sets);
  if (np == 0) return TRGT_OK;
  if (!in->motif_blob || !in->motif_off || !in->set_motif_begin || !in->panel_set || !in->ref_blob || !in->ref_off || !in->ref_len || !in->lf_len || !in->rf_len || !in->panel_read_begin)
    return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: null field (in: motif_blob, motif_off, set_motif_begin, panel_set, ref_blob, ref_off, ref_len, lf_len, rf_len, panel_read_begin)");
  if (mode == 0 && (!out->pseg || !out->pseg_off || !out->n_pseg)) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: null field (out: pseg, pseg_off, n_pseg are required in mode 0)");
  try {
    if (c->knobs.timeline) c->tl_t0 = wall_ns();   // (TRGT_TIMELINE: the call's host-side phases on stderr)
    // ---- the checks: everything the kernels index with is checked here, on the host, before the first launch and the first output
    const uint64_t* prb = in->panel_read_begin;
    if (prb[0] != 0) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: panel_read_begin must start at 0");
    for (int64_t p = 0; p < np; ++p) if (prb[p] > prb[p + 1]) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: panel_read_begin decreases at panel %lld", (long long)p);
    const uint64_t nr = prb[np];
    if (nr > 0x3FFFFFF0ull) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_plot_align_batch: too many reads in one call");
    if (nr && (!in->read_blob || !in->read_off || !in->read_len || !out->rseg || !out->rseg_off || !out->n_rseg))
      return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: null field (in: read_blob, read_off, read_len; out: rseg, rseg_off, n_rseg)");
    const uint64_t n_beta = in->beta_begin ? in->beta_begin[nr] : 0;
    if (n_beta && !in->beta_pos) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: null field (in: beta_pos)");
    if (n_beta > 0x7FFFFFF0ull) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_plot_align_batch: too many betas in one call");
    constexpr uint64_t MAX_SUM = 1ull << 27;   // what one alignment of the batch aligner may span
    uint64_t ref_lo = ~0ull, ref_hi = 0, read_lo = ~0ull, read_hi = 0;
    for (int64_t p = 0; p < np; ++p) {
      if ((int64_t)in->panel_set[p] >= (int64_t)in->n_sets) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: panel %lld has motif set %u of %d", (long long)p, in->panel_set[p], in->n_sets);
      const uint64_t fl = (uint64_t)in->lf_len[p] + in->rf_len[p];
      if (mode == 0 ? in->ref_len[p] < fl : in->ref_len[p] != fl)
        return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: panel %lld has ref_len %u with flanks of %u + %u bases (%s)", (long long)p, in->ref_len[p], in->lf_len[p], in->rf_len[p],
                    mode == 0 ? "the consensus holds both flanks" : "a waterfall reference is the two flanks");
      if (mode == 0 && in->ref_len[p] == 0) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: panel %lld has an empty consensus", (long long)p);
      if (in->ref_len[p]) { ref_lo = std::min(ref_lo, in->ref_off[p]); ref_hi = std::max(ref_hi, in->ref_off[p] + in->ref_len[p]); }
      for (uint64_t r = prb[p]; r < prb[p + 1]; ++r) {
        const uint64_t len = in->read_len[r];
        if (mode == 1 && len < fl) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: read %llu of panel %lld has %u bases, fewer than its flanks of %u + %u", (unsigned long long)r, (long long)p, in->read_len[r], in->lf_len[p], in->rf_len[p]);
        if (mode == 0 && len == 0) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: read %llu of panel %lld is empty", (unsigned long long)r, (long long)p);
        if ((mode == 0 ? len + in->ref_len[p] : len) > MAX_SUM) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_plot_align_batch: read %llu of panel %lld is beyond the aligner's 2^27 bases per alignment", (unsigned long long)r, (long long)p);
        if (len) { read_lo = std::min(read_lo, in->read_off[r]); read_hi = std::max(read_hi, in->read_off[r] + len); }
      }
      if (in->ref_len[p] > MAX_SUM) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_plot_align_batch: panel %lld is beyond the aligner's 2^27 bases per alignment", (long long)p);
    }
    if (ref_hi <= ref_lo) ref_lo = ref_hi = 0;
    if (read_hi <= read_lo) read_lo = read_hi = 0;
    TRGT_HIP_TRY(c, hipSetDevice(c->device));
    const bool ref_dev = is_device_ptr(in->ref_blob), read_dev = nr && is_device_ptr(in->read_blob);
    std::vector<uint8_t> keep_ref, keep_read;
    const uint8_t *h_ref = nullptr, *h_read = nullptr;
    int rc;
    if ((rc = plot::host_view(c, in->ref_blob, ref_dev, ref_lo, ref_hi, keep_ref, &h_ref)) || (rc = plot::host_view(c, in->read_blob, read_dev, read_lo, read_hi, keep_read, &h_read))) return rc;
    for (int64_t p = 0; p < np; ++p) {
      const size_t i = plot::first_not_acgt(h_ref + in->ref_off[p], in->ref_len[p]);
      if (i < in->ref_len[p]) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: the reference of panel %lld has byte 0x%02x at position %zu (not one of ACGT)", (long long)p, h_ref[in->ref_off[p] + i], i);
    }
    for (uint64_t r = 0; r < nr; ++r) {
      const size_t i = plot::first_not_acgt(h_read + in->read_off[r], in->read_len[r]);
      if (i < in->read_len[r]) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: read %llu has byte 0x%02x at position %zu (not one of ACGT)", (unsigned long long)r, h_read[in->read_off[r] + i], i);
    }
    const uint32_t m_total = in->set_motif_begin[in->n_sets];
    for (int32_t s = 0; s < in->n_sets; ++s)
      for (uint32_t m = in->set_motif_begin[s]; m < in->set_motif_begin[s + 1]; ++m)
        for (uint32_t i = in->motif_off[m]; i < in->motif_off[m + 1]; ++i)
          if (!plot::is_acgt(in->motif_blob[i]) && in->motif_blob[i] != 'N') return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: motif %u of set %d has byte 0x%02x (not one of ACGTN)", m - in->set_motif_begin[s], s, in->motif_blob[i]);
    (void)m_total;
    if (in->beta_begin)
      for (uint64_t r = 0; r < nr; ++r) {
        if (in->beta_begin[r] > in->beta_begin[r + 1]) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: beta_begin decreases at read %llu", (unsigned long long)r);
        const uint32_t* q = in->beta_pos + in->beta_begin[r];
        const uint64_t nq = in->beta_begin[r + 1] - in->beta_begin[r];
        uint32_t bad = nq && q[0] >= in->read_len[r];
        for (uint64_t i = 1; i < nq; ++i) bad |= (uint32_t)(q[i] >= in->read_len[r]) | (uint32_t)(q[i] <= q[i - 1]);
        if (!bad) continue;   // (else: name the first offender)
        for (uint64_t i = in->beta_begin[r]; i < in->beta_begin[r + 1]; ++i) {
          if (in->beta_pos[i] >= in->read_len[r]) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: read %llu has a beta at position %u, beyond its %u bases", (unsigned long long)r, in->beta_pos[i], in->read_len[r]);
          if (i > in->beta_begin[r] && in->beta_pos[i] <= in->beta_pos[i - 1]) return fail(c, TRGT_ERR_INVALID, "trgt_plot_align_batch: the betas of read %llu are not strictly increasing (%u behind %u)", (unsigned long long)r, in->beta_pos[i], in->beta_pos[i - 1]);
        }
      }
    // (the model limits: 4 096 states, 253 motifs -- the device builder checks them on the host before it uploads or launches anything)
    tl_mark(c, "plot: checked");
    HmmModels models;
    {
      const int mrc = hmm_models_on_device(c, in->n_sets, in->motif_blob, in->motif_off, in->set_motif_begin, models, c->stream, nullptr);
      if (mrc) return fail(c, mrc, "%s", models.err.empty() ? trgt_hip_last_error(c) : models.err.c_str());
    }

    // ---- the plan: items of both kernels, jobs of both batches, the layout of slab and workspace
    const uint64_t ref_bytes = ref_hi - ref_lo, read_bytes = read_hi - read_lo;
    const uint64_t o_ref = 0, o_read = (ref_bytes + 63) & ~63ull;
    auto ref_at = [&](int64_t p) { return o_ref + (in->ref_off[p] - ref_lo); };
    auto read_at = [&](uint64_t r) { return o_read + (in->read_off[r] - read_lo); };
    const size_t n_mitems = mode == 0 ? (size_t)np : (size_t)nr;
    std::vector<plot::MotifItem> mitems(n_mitems);
    std::vector<plot::ReadItem> ritems((size_t)nr);
    std::vector<uint32_t> h_set, h_len; std::vector<uint64_t> h_soff, h_poff, h_coff;   // the HMM batch
    uint64_t path_total = 0, tbb_total = 0, wseg_total = 0, run_total = 0, count_total = 0;
    auto add_item = [&](size_t i, uint32_t set, uint64_t seq_off, uint32_t len, uint32_t lf, uint32_t rf, uint64_t seg_off) {
      plot::MotifItem& it = mitems[i];
      it = plot::MotifItem{};
      it.seq_off = seq_off; it.seq_len = len; it.set = set; it.lf = lf; it.rf = rf; it.hjob = -1;
      it.tbb_off = tbb_total; tbb_total += (uint64_t)len + 2;
      if (mode == 0) { it.seg_off = seg_off; it.run_off = run_total; run_total += (uint64_t)len + 2; }
      else { it.seg_off = wseg_total; wseg_total += 2ull * len + 1; }
      if (len == 0) return;
      const HmmSetDev& sd = models.sets[set];
      it.hjob = (int32_t)h_set.size();
      it.path_off = path_total; it.path_cap = (uint32_t)std::min<uint64_t>(trgt_hmm_path_capacity(len, sd.max_mlen), 0xFFFFFFFFull);
      h_set.push_back(set); h_len.push_back(len); h_soff.push_back(seq_off); h_poff.push_back(path_total); h_coff.push_back(count_total);
      path_total += it.path_cap; count_total += sd.n_blocks - 1;
    };
    std::vector<uint64_t> pat_off, txt_off; std::vector<uint32_t> pat_len, txt_len;   // the alignment batch
    auto add_job = [&](uint64_t po, uint32_t pl, uint64_t to, uint32_t tl) { pat_off.push_back(po); pat_len.push_back(pl); txt_off.push_back(to); txt_len.push_back(tl); return (int32_t)(pat_off.size() - 1); };
    uint64_t pseg_words = 0, rseg_words = 0;
    for (int64_t p = 0; p < np; ++p) {
      const uint32_t lf = in->lf_len[p], rf = in->rf_len[p], set = in->panel_set[p];
      uint32_t longest = 0;
      for (uint64_t r = prb[p]; r < prb[p + 1]; ++r) longest = std::max(longest, in->read_len[r]);
      if (mode == 0) {
        add_item((size_t)p, set, ref_at(p) + lf, in->ref_len[p] - lf - rf, lf, rf, out->pseg_off[p]);
        pseg_words = std::max<uint64_t>(pseg_words, 2 * (out->pseg_off[p] + plot::seg_capacity(0, in->ref_len[p], 0)));
      }
      for (uint64_t r = prb[p]; r < prb[p + 1]; ++r) {
        plot::ReadItem& it = ritems[(size_t)r];
        it = plot::ReadItem{};
        const uint32_t len = in->read_len[r];
        it.rseg_off = out->rseg_off[r]; it.read_len = len; it.ref_len = in->ref_len[p];
        const uint64_t cap = plot::seg_capacity(mode, in->ref_len[p], len);
        it.cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull);
        rseg_words = std::max<uint64_t>(rseg_words, 2 * (out->rseg_off[r] + cap));
        const uint64_t b0 = in->beta_begin ? in->beta_begin[r] : 0, b1 = in->beta_begin ? in->beta_begin[r + 1] : 0;
        it.beta_off = b0; it.n_beta = (uint32_t)(b1 - b0);
        it.job[0] = it.job[1] = -1;
        if (mode == 0) {
          it.item = (uint32_t)p; it.run_off = mitems[(size_t)p].run_off;
          it.job[0] = add_job(ref_at(p), in->ref_len[p], read_at(r), len);
        } else {
          const uint32_t tr = len - lf - rf;
          add_item((size_t)r, set, read_at(r) + lf, tr, lf, rf, 0);
          it.item = (uint32_t)r; it.tr_seg_off = mitems[(size_t)r].seg_off; it.lf = lf; it.tr = tr; it.pad_w = longest - len;
          if (lf) it.job[0] = add_job(ref_at(p), lf, read_at(r), lf);
          if (rf) it.job[1] = add_job(ref_at(p) + lf, rf, read_at(r) + lf + tr, rf);
          const uint32_t* bp = in->beta_pos + b0;
          it.nb_lf = (uint32_t)(std::lower_bound(bp, bp + it.n_beta, lf) - bp);
          it.nb_tr = (uint32_t)(std::lower_bound(bp, bp + it.n_beta, lf + tr) - bp);
        }
      }
    }
    const size_t nhj = h_set.size(), nwj = pat_off.size();
    if (n_mitems > 0xFFFFFFF0ull / 4) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_plot_align_batch: too many panels in one call");

    tl_mark(c, "plot: planned");
    // ---- one upload: reference bytes | read bytes | items of both kernels | beta positions
    struct Lay { size_t total = 0; size_t add(size_t b) { const size_t o = (total + 63) & ~(size_t)63; total = o + b; return o; } } lay;
    lay.add((size_t)o_read + (size_t)read_bytes);
    const size_t o_mitems = lay.add(n_mitems * sizeof(plot::MotifItem)), o_ritems = lay.add((size_t)nr * sizeof(plot::ReadItem)), o_beta = lay.add((size_t)n_beta * 4);
    void* d_in = nullptr;
    if ((rc = dev_get(c, S_PLOT_IN, lay.total + 64, &d_in))) return rc;
    uint8_t* const d_slab = (uint8_t*)d_in;
    {
      // (each piece straight from where it is: a copy from pageable memory returns once its bytes are staged, and the item lists live to
      //  the end of the call; blobs in HBM are copied there)
      auto up = [&](size_t at, const void* src, size_t bytes, bool src_dev) -> hipError_t {
        return bytes ? hipMemcpyAsync(d_slab + at, src, bytes, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream) : hipSuccess;
      };
      TRGT_HIP_TRY(c, up((size_t)o_ref, in->ref_blob + ref_lo, (size_t)ref_bytes, ref_dev));
      TRGT_HIP_TRY(c, up((size_t)o_read, nr ? in->read_blob + read_lo : nullptr, (size_t)read_bytes, read_dev));
      TRGT_HIP_TRY(c, up(o_mitems, mitems.data(), n_mitems * sizeof(plot::MotifItem), false));
      TRGT_HIP_TRY(c, up(o_ritems, ritems.data(), (size_t)nr * sizeof(plot::ReadItem), false));
      TRGT_HIP_TRY(c, up(o_beta, in->beta_pos, (size_t)n_beta * 4, false));
    }
    // ---- workspace: motif_by_base | repeat-part segments (mode 1) | seg-type runs (mode 0) | counts | flag
    Lay wl;
    const size_t w_tbb = wl.add((size_t)tbb_total * 2), w_seg = wl.add((size_t)wseg_total * 8), w_runs = wl.add((size_t)run_total * 8), w_ntr = wl.add(n_mitems * 4),
                 w_nruns = wl.add(n_mitems * 4), w_flag = wl.add(16);
    void *d_work = nullptr, *d_path = nullptr, *d_hout = nullptr, *d_wout = nullptr;
    Lay hl;
    const size_t h_pur = hl.add(nhj * 8), h_plen = hl.add(nhj * 4), h_nsp = hl.add(nhj * 4), h_cnt = hl.add((size_t)count_total * 4);
    if ((rc = dev_get(c, S_PLOT_WORK, wl.total + 64, &d_work)) || (rc = dev_get(c, S_PLOT_PATH, (size_t)path_total * 2 + 64, &d_path)) ||
        (rc = dev_get(c, S_PLOT_HMMOUT, hl.total + 64, &d_hout)) || (rc = dev_get(c, S_PLOT_WFAOUT, nwj * 8 + 64, &d_wout)))
      return rc;
    uint8_t* const wk = (uint8_t*)d_work;
    TRGT_HIP_TRY(c, hipMemsetAsync(wk + w_flag, 0xFF, 16, c->stream));
    DevOut<uint32_t> o_pseg, o_npseg, o_rseg, o_nrseg; DevOut<int32_t> o_bproj, o_score;
    if (mode == 0 && ((rc = o_pseg.init(c, S_PLOT_PSEG, out->pseg, (size_t)pseg_words)) || (rc = o_npseg.init(c, S_PLOT_NPSEG, out->n_pseg, (size_t)np)))) return rc;
    if (nr && ((rc = o_rseg.init(c, S_PLOT_RSEG, out->rseg, (size_t)rseg_words)) || (rc = o_nrseg.init(c, S_PLOT_NRSEG, out->n_rseg, (size_t)nr)) ||
               (rc = o_bproj.init(c, S_PLOT_BPROJ, n_beta ? out->beta_proj : nullptr, (size_t)n_beta)) || (rc = o_score.init(c, S_PLOT_SCORE, out->score, (size_t)nr))))
      return rc;
    // (pseg / rseg in host memory: the kernels fill device slots of the same layout, and only their used parts come back -- copy-out, below)

    tl_mark(c, "plot: uploaded");
    // ---- Hmm::label of every repeat, the paths left in HBM (spans stay in the batch's own tight layout; counts and purities
    // have to go somewhere: trgt_hmm_batch requires them)
    if (nhj) {
      HmmBatchIO io;
      io.n_sets = in->n_sets; io.motif_blob = in->motif_blob; io.motif_off = in->motif_off; io.set_motif_begin = in->set_motif_begin;
      io.n_jobs = (int64_t)nhj; io.job_set = h_set.data(); io.seq_blob = d_slab; io.seq_off = h_soff.data(); io.seq_len = h_len.data();
      io.path = (uint16_t*)d_path; io.path_off = h_poff.data(); io.path_len = (uint32_t*)((uint8_t*)d_hout + h_plen);
      io.spans3 = nullptr; io.n_spans = (uint32_t*)((uint8_t*)d_hout + h_nsp);
      io.motif_counts = (uint32_t*)((uint8_t*)d_hout + h_cnt); io.count_off = h_coff.data(); io.purity = (double*)((uint8_t*)d_hout + h_pur);
      if ((rc = hmm_batch_impl(c, &models, io))) return rc;
    }
    tl_mark(c, "plot: HMM batch done");
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (c->timing) for (auto& e : ev) TRGT_HIP_TRY(c, hipEventCreate(&e));
    // ---- plot_motif_segs_kernel
    if (n_mitems) {
      plot::MotifArgs ma{};
      ma.items = (const plot::MotifItem*)(d_slab + o_mitems); ma.n_items = (uint32_t)n_mitems; ma.mode = mode;
      ma.slab = d_slab; ma.path = (const uint16_t*)d_path; ma.path_len = (const uint32_t*)((uint8_t*)d_hout + h_plen);
      ma.sets = (const HmmSetDev*)models.d_sets; ma.model = (const uint8_t*)models.d_blob;
      ma.tbb = (uint16_t*)(wk + w_tbb); ma.work_seg = (uint32_t*)(wk + w_seg); ma.runs = (uint32_t*)(wk + w_runs);
      ma.n_tr = (uint32_t*)(wk + w_ntr); ma.n_runs = (uint32_t*)(wk + w_nruns); ma.pseg = o_pseg.dev; ma.n_pseg = o_npseg.dev;
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[0], c->stream));
      hipLaunchKernelGGL(plot::plot_motif_segs_kernel, dim3((unsigned)((n_mitems + 3) / 4)), dim3(256), 0, c->stream, ma);
      TRGT_HIP_TRY(c, hipGetLastError());
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[1], c->stream));
    }
    // ---- the alignments: WFAligner::builder(Alignment, MemoryHigh).affine(2, 5, 1), the default heuristic; CIGARs stay in HBM
    WfaOnDevice od;
    int32_t* const d_status = (int32_t*)d_wout; int32_t* const d_wscore = d_status + nwj;
    if (nwj) {
      trgt_wfa_params wp;
      trgt_wfa_default_params(&wp);
      wp.metric = 3; wp.mismatch = 2; wp.gap_open1 = 5; wp.gap_ext1 = 1; wp.span = 0; wp.scope = 1; wp.memory_mode = 0;
      WfaBatchIO io;
      io.n_jobs = (int64_t)nwj; io.seqs = d_slab; io.pat_off = pat_off.data(); io.pat_len = pat_len.data(); io.txt_off = txt_off.data(); io.txt_len = txt_len.data();
      io.status = d_status; io.score = d_wscore; io.on_device = &od;
      if ((rc = wfa_batch_impl(c, &wp, io))) return rc;
    }
    tl_mark(c, "plot: alignment batch done");
    // ---- plot_read_segs_kernel, behind the batch on the same stream (WfaOnDevice holds until the context's next alignment batch)
    if (nr) {
      plot::ReadArgs ra{};
      ra.items = (const plot::ReadItem*)(d_slab + o_ritems); ra.n_items = (uint32_t)nr; ra.mode = mode;
      ra.jobs = od.jobs; ra.cigar = od.cigar; ra.cigar_len = od.cigar_len; ra.status = d_status; ra.wfa_score = d_wscore;
      ra.runs = (const uint32_t*)(wk + w_runs); ra.n_runs = (const uint32_t*)(wk + w_nruns); ra.work_seg = (const uint32_t*)(wk + w_seg); ra.n_tr = (const uint32_t*)(wk + w_ntr);
      ra.beta_pos = (const uint32_t*)(d_slab + o_beta); ra.beta_proj = o_bproj.dev; ra.rseg = o_rseg.dev; ra.n_rseg = o_nrseg.dev; ra.score = o_score.dev;
      ra.flag = (unsigned int*)(wk + w_flag);
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[2], c->stream));
      hipLaunchKernelGGL(plot::plot_read_segs_kernel, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, c->stream, ra);
      TRGT_HIP_TRY(c, hipGetLastError());
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[3], c->stream));
    }
    // ---- copy-out
    uint32_t flag = 0xFFFFFFFFu;
    std::vector<int32_t> h_score;
    const bool want_scores = out->order && mode == 0 && nr;
    if (want_scores) { h_score.resize(nwj); if ((rc = d2h(c, h_score.data(), d_wscore, nwj * 4, c->stream))) return rc; }
    std::vector<uint32_t> h_np, h_nr;   // segment counts, for the segments that go to host arrays
    if (o_pseg.staged) { h_np.resize((size_t)np); if ((rc = d2h(c, h_np.data(), o_npseg.dev, (size_t)np * 4, c->stream))) return rc; }
    if (o_rseg.staged) { h_nr.resize((size_t)nr); if ((rc = d2h(c, h_nr.data(), o_nrseg.dev, (size_t)nr * 4, c->stream))) return rc; }
    if ((rc = d2h(c, &flag, wk + w_flag, 4, c->stream)) || (rc = o_npseg.finish(c)) || (rc = o_nrseg.finish(c)) || (rc = o_bproj.finish(c)) || (rc = o_score.finish(c))) return rc;
    TRGT_HIP_TRY(c, trgt::stream_wait(c, c->stream));
    tl_mark(c, "plot: kernels done");
    if (flag == 0xFFFFFFFFu && (h_np.size() || h_nr.size())) {
      // the used part of every slot, packed on the device, one copy, then slot by slot into the caller's array
      std::vector<uint64_t> poff(h_np.size() + h_nr.size() + 1, 0);
      for (size_t i = 0; i < h_np.size(); ++i) poff[i + 1] = poff[i] + h_np[i];
      for (size_t i = 0; i < h_nr.size(); ++i) poff[h_np.size() + i + 1] = poff[h_np.size() + i] + h_nr[i];
      const uint64_t total = poff.back();
      void *d_poff = nullptr, *d_packed = nullptr;
      if ((rc = dev_get(c, S_PLOT_POFF, poff.size() * 8, &d_poff)) || (rc = dev_get(c, S_PLOT_PACKED, (size_t)total * 8 + 16, &d_packed)) ||
          (rc = h2d_small(c, d_poff, poff.data(), poff.size() * 8, c->stream, S_PLOT_POFF)))
        return rc;
      if (h_np.size())
        hipLaunchKernelGGL(plot::plot_pack_segs_kernel, dim3((unsigned)((h_np.size() + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t*)o_pseg.dev, d_slab + o_mitems,
                           (uint32_t)sizeof(plot::MotifItem), (uint32_t)offsetof(plot::MotifItem, seg_off), (uint32_t)h_np.size(), (const uint32_t*)o_npseg.dev, (const uint64_t*)d_poff, (uint32_t*)d_packed);
      if (h_nr.size())
        hipLaunchKernelGGL(plot::plot_pack_segs_kernel, dim3((unsigned)((h_nr.size() + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t*)o_rseg.dev, d_slab + o_ritems,
                           (uint32_t)sizeof(plot::ReadItem), (uint32_t)offsetof(plot::ReadItem, rseg_off), (uint32_t)h_nr.size(), (const uint32_t*)o_nrseg.dev,
                           (const uint64_t*)d_poff + h_np.size(), (uint32_t*)d_packed);
      TRGT_HIP_TRY(c, hipGetLastError());
      std::vector<uint32_t> h_packed((size_t)total * 2);
      if (total) { if ((rc = d2h(c, h_packed.data(), d_packed, (size_t)total * 8, c->stream))) return rc; }
      TRGT_HIP_TRY(c, trgt::stream_wait(c, c->stream));
      for (size_t i = 0; i < h_np.size(); ++i) if (h_np[i]) std::memcpy(out->pseg + 2 * out->pseg_off[i], h_packed.data() + 2 * poff[i], (size_t)h_np[i] * 8);
      for (size_t i = 0; i < h_nr.size(); ++i) if (h_nr[i]) std::memcpy(out->rseg + 2 * out->rseg_off[i], h_packed.data() + 2 * poff[h_np.size() + i], (size_t)h_nr[i] * 8);
    }
    if (c->timing) {
      float ms = 0;
      c->plot_ms[0] = n_mitems && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess ? ms : 0.0;
      c->plot_ms[1] = nr && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess ? ms : 0.0;
      (void)hipGetLastError();
      for (auto& e : ev) c->retired_events.push_back(e);
    } else c->plot_ms[0] = c->plot_ms[1] = 0.0;
    if (flag != 0xFFFFFFFFu) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_plot_align_batch: an alignment of read %u did not complete", flag);
    tl_mark(c, "plot: outputs copied");
    // ---- the drawing order: align_reads.rs:26 (read length, then the higher score first), waterfall_plot.rs:28-31 (read length); both stable
    if (out->order && nr) {
      std::vector<uint32_t> ord((size_t)nr);
      std::iota(ord.begin(), ord.end(), 0u);
      for (int64_t p = 0; p < np; ++p)
        std::stable_sort(ord.begin() + (ptrdiff_t)prb[p], ord.begin() + (ptrdiff_t)prb[p + 1], [&](uint32_t x, uint32_t y) {
          if (in->read_len[x] != in->read_len[y]) return in->read_len[x] < in->read_len[y];
          return mode == 0 && h_score[x] > h_score[y];
        });
      if (is_device_ptr(out->order)) TRGT_HIP_TRY(c, hipMemcpy(out->order, ord.data(), (size_t)nr * 4, hipMemcpyHostToDevice));
      else std::memcpy(out->order, ord.data(), (size_t)nr * 4);
    }
    return TRGT_OK;
  } catch (const std::bad_alloc&) { return fail(c, TRGT_ERR_NOMEM, "out of host memory"); }
}
