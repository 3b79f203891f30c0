// trgt_amd/csrc/wfa_host.hpp -- job record and host-side launch descriptor of the WFA kernel (no device code).
#pragma once
#include <functional>
#include <vector>
#include "common.hpp"
#include "wfa_types.hpp"  // JobDev

namespace trgt {

// A read shorter than this cannot contain the repeat of its locus with both flanks around it (the longest read of the locus is
// the yardstick): at least one of its flank alignments ends with a long gap, i.e. runs through many score levels.
inline uint32_t heavy_read_len(uint32_t locus_max_read_len, int flank_len) {
  const uint32_t margin = (uint32_t)flank_len + (uint32_t)flank_len / 5;
  return locus_max_read_len > margin ? locus_max_read_len - margin : 0;
}

// The --aln-scoring presets of the reference (cli.rs:271-280): 2,5,1 (wgs) is the configuration the specialised kernels are compiled
// for; the pre-filter (wfa_reg.hip) has an instantiation for 1,0,1 (targeted) as well.
inline bool preset_wgs(int mism, int gapo, int gape) { return mism == 2 && gapo == 5 && gape == 1; }
inline bool preset_has_filter(int mism, int gapo, int gape) { return preset_wgs(mism, gapo, gape) || (mism == 1 && gapo == 0 && gape == 1); }

struct WfaLaunch {  // everything device-resident
  const JobDev* jobs_dev = nullptr; int64_t n_jobs_host = 0; const uint32_t* n_jobs_dev = nullptr;
  int64_t jobs_bound = 0;  // with n_jobs_dev: the most jobs the list can hold (0: n_jobs_host is that bound, not just a bound on the workgroups)
  // two-ended list: jobs expected to be expensive are appended from the front (count *n_jobs_dev) and are drained first,
  // the others from the back (jobs_dev[jobs_cap - 1 - k], count *n_jobs2_dev)
  const uint32_t* n_jobs2_dev = nullptr; uint32_t jobs_cap = 0;
  const uint8_t* pat_base = nullptr; const uint8_t* txt_base = nullptr;
  int64_t max_plen = 0, max_tlen = 0, max_sum = 0;
  int threads = 0;
  int timer_slot = TRGT_K_WFA;
  int max_score = 0;    // > 0: alignments whose penalty exceeds it are given up (status OOM, score INT32_MIN): with pattern_begin_free = 0 and a
                        // fixed text_begin_free the wavefronts then stay within [-max_score, text_begin_free + max_score] and the LDS ring of the
                        // dedicated kernel is sized (and indexed) for that range instead of the whole text
  int kernel_tag = -1;  // instantiation of the dedicated kernel to launch (-1: 1 for timer_slot == TRGT_K_WFA_FLANK_REST, else 0); names the launch in a trace
  bool keep_cells = false;  // do not reset the wavefront-offset counter (a second launch of the same logical batch)
  uint64_t ws_budget = 0;  // > 0: the generic kernel's workgroups (one workspace each) are limited to this many bytes of workspace -- launches whose jobs
                           // the register-resident kernels take almost entirely, planned for lengths far above what the jobs have
  int buffer_set = 0;  // 0 / 1 / 2: which workspace / counter buffers of the ctx to use (launches may be in flight on two streams; 2 = the device-side consensus repair, whose buffers must not be re-sized while the flank location is still running on sets 0 / 1)
  int32_t* status = nullptr; int32_t* score = nullptr; int32_t* n_match = nullptr; uint32_t* span4 = nullptr;
  uint32_t* cigar = nullptr; uint32_t* cigar_len = nullptr; uint8_t* ops = nullptr; uint32_t* ops_len = nullptr;
  unsigned int* refused = nullptr;  // device word that counts the jobs the kernel refuses (longer than the planned workspace): device-built lists carry one
                                    // that comes back with the call's count block, so that such a job fails the call instead of leaving an INT32_MIN behind
};

// Enqueue the WFA kernel on the ctx stream (asynchronous).  The number of wavefront offsets computed is
// accumulated in device memory at ctx->last_wfa_cells_dev.
int wfa_launch(trgt_hip_ctx* c, const trgt_wfa_params& p, const WfaLaunch& L);

// The windowed flank alignments of trgt_find_spans_batch on one wave each, wavefronts and history in registers (wfa_win.hip): gap-affine
// (2, 5, 1), pattern ends fixed, text free at both ends, started on the diagonals [0, tbf], given up above the penalty s_max.  Writes
// score (-penalty, INT32_MIN when given up or not taken), n_match and span4 by JobDev::out_index, exactly as wfa_launch with
// kernel_tag 2 and max_score = s_max does for the alignments that come out at s_max or below.
struct WfaWinLaunch {
  const JobDev* jobs_dev = nullptr; int64_t n_jobs_host = 0; const uint32_t* n_jobs_dev = nullptr;
  const uint8_t* pat_base = nullptr; const uint8_t* txt_base = nullptr;
  int tbf = 0, s_max = 0;
  unsigned int* counter = nullptr;   // cleared device word: job claims
  unsigned int* fallback = nullptr;  // device word that counts the jobs the kernel does not take (sequences beyond its staging buffers)
  int32_t* score = nullptr; int32_t* n_match = nullptr; uint32_t* span4 = nullptr;
  int timer_slot = TRGT_K_WFA_FLANK_REST;
};
// wfa_win_fits: can the kernel hold a launch with these parameters at all (else: wfa_launch)
bool wfa_win_fits(int mism, int gapo, int gape, int tbf, int s_max, int64_t max_plen, int64_t max_tlen);
int wfa_win_launch(trgt_hip_ctx* c, const WfaWinLaunch& L);

// The banded alignments of what the pre-filter keeps, one wave each and forward only (wfa_band.hip): gap-affine (2, 5, 1).  The kernel reads
// the kept list itself (penalty s* and end diagonal in JobDev::pad), aligns each piece inside its band and writes n_match and span4 of the
// jobs that come out at s* with matches.  The others go to rest_jobs (whole read; counted in count[i_fail] where a banded run did not
// stand), and banded jobs its layout cannot hold (s* > WFA_BAND_S_CAP, a piece beyond WFA_BAND_PLEN_MAX) to fall_jobs for wfa_launch.
constexpr int WFA_BAND_S_CAP = 96, WFA_BAND_PLEN_MAX = 255;
struct WfaBandLaunch {
  const JobDev* jobs_dev = nullptr; int64_t n_jobs_host = 0; const uint32_t* n_jobs_dev = nullptr;
  const uint8_t* pat_base = nullptr; const uint8_t* txt_base = nullptr;
  uint32_t* count = nullptr;  // the call's cleared counter block, and the words of it: job claims, jobs taken, lengths of the two lists, failures
  int i_claim = 0, i_reg = 0, i_fall = 0, i_rest = 0, i_fail = 0;
  JobDev* fall_jobs = nullptr; JobDev* rest_jobs = nullptr;
  int32_t* n_match = nullptr; uint32_t* span4 = nullptr;
  const uint64_t* read_off = nullptr; const uint32_t* read_len = nullptr;  // by read (out_index / 2): the whole read of a job that did not stand
  int s_max = 0;  // jobs whose penalty exceeds it are not banded at all
  int timer_slot = TRGT_K_WFA_FLANK;
};
int wfa_band_launch(trgt_hip_ctx* c, const WfaBandLaunch& L);

// The register-resident BiWFA kernel for small end-to-end alignments (wfa_lean.hip), launched by wfa_launch in front of the generic
// kernel: alignments it does not take are appended to retry_jobs / *retry_count (device memory) and redone there from scratch.
int wfa_lean_launch(trgt_hip_ctx* c, const trgt_wfa_params& p, const WfaLaunch& L, JobDev* mid_jobs, JobDev* retry_jobs, unsigned int* retry_count, uint32_t retry_cap,
                    unsigned int* retry_lost, unsigned int* counters, unsigned long long* cells_out, unsigned int* why_hist);

// ---- register-resident pre-filter of the flank fallback alignments (wfa_reg.hip) ----
struct FilterArgs {  // by-value kernel argument
  const JobDev* jobs; const uint32_t* n_jobs_dev; uint32_t n_jobs;
  const uint8_t* pat_base; const uint8_t* txt_base;
  unsigned int* counter;
  int32_t min_matches;                      // an alignment is kept iff its match bound >= min_matches (or it could not be judged)
  int32_t early_reject;                     // stop an alignment as soon as no cell of its wavefronts can reach min_matches any more
  JobDev* keep_jobs; uint32_t* keep_count;  // kept alignments, appended (NULL: none wanted)
  int32_t* score; int32_t* bound; uint8_t* keep;  // optional, indexed by JobDev::out_index
  uint32_t* band;                           // optional, by out_index: bit 31 | penalty << 16 | biased end diagonal of a run that completed; bit 30 | level of one rejected early (its penalty is larger); 0: not judged
  int32_t diag_lo, diag_hi;                 // this launch takes the jobs with diag_lo < plen + tlen + 1 <= diag_hi (the others belong to another launch over the same list)
  unsigned long long* cells_out;
};
struct FilterLaunch {
  const JobDev* jobs_dev = nullptr; int64_t n_jobs_host = 0; const uint32_t* n_jobs_dev = nullptr;
  const uint8_t* pat_base = nullptr; const uint8_t* txt_base = nullptr;
  int64_t max_plen = 0, max_tlen = 0;
  int32_t min_matches = 0;
  int mism = 2, gapo = 5, gape = 1;  // --aln-scoring: 2,5,1 (wgs) or 1,0,1 (targeted) have an instantiation
  bool early_reject = false;  // see FilterArgs (then: score INT32_MIN + 1, bound min_matches - 1 for the alignments stopped early)
  JobDev* keep_jobs = nullptr; uint32_t* keep_count = nullptr;
  int32_t* score = nullptr; int32_t* bound = nullptr; uint8_t* keep = nullptr; uint32_t* band = nullptr;
  bool count_offsets = false;  // also count the wavefront offsets (a little slower: one more scalar walk per level)
  int timer_slot = TRGT_K_WFA_FILTER;
  int set = 0;  // 1: a second launch that may run next to the first (own job counter and offset counter; ctx->last_filter_cells_dev stays the first's)
};
// Longest text the filter can judge for this pattern length (0: the filter does not apply); longer texts are kept unseen.
int flank_filter_max_tlen(int flank_len);
// Enqueue the filter on the ctx stream (asynchronous); offsets computed are accumulated at ctx->last_filter_cells_dev.
int flank_filter_launch(trgt_hip_ctx* c, const FilterLaunch& L);

// ---- flank location (spans.hip) ----
// The device-side part of trgt_find_spans_batch, shared with trgt_locus_batch: everything already resident, results left on the device.
int find_spans_device(trgt_hip_ctx* c, const trgt_span_params& p, int64_t n_reads, const uint8_t* d_flank, const uint64_t* d_piece_off,
                      const uint8_t* d_reads, const uint64_t* d_read_off, const uint32_t* d_read_len, const uint32_t* d_read_locus,
                      uint32_t max_read_len, int32_t* d_span_start, int32_t* d_span_end, uint8_t* d_lf_hit, uint8_t* d_rf_hit,
                      const uint32_t* d_heavy_len, uint32_t heavy_tlen_max, bool span_only);

// Run-length CIGARs of a whole batch in one dense array: job j = data[off[j] .. off[j + 1]) (len << 4 | code, as cigar_get_CIGAR).
struct PackedCigars { std::vector<uint32_t> data; std::vector<uint64_t> off; };
// ... or left in HBM for a kernel of the caller (the consensus column voting): job list, CIGAR slots (job j at cigar[jobs[j].cigar_off ..],
// cigar_len[jobs[j].out_index] entries) and the sequence blob, valid until the next alignment batch of the context
struct WfaOnDevice { const JobDev* jobs = nullptr; const uint32_t* cigar = nullptr; const uint32_t* cigar_len = nullptr; const uint8_t* seqs = nullptr; };
// The caller's arrays of an alignment batch, as trgt_wfa_batch (include/trgt_hip.h) documents them, and what the internal callers add.
struct WfaBatchIO {
  int64_t n_jobs = 0; const uint8_t* seqs = nullptr;
  const uint64_t* pat_off = nullptr; const uint32_t* pat_len = nullptr; const uint64_t* txt_off = nullptr; const uint32_t* txt_len = nullptr;
  int32_t* status = nullptr; int32_t* score = nullptr; int32_t* n_match = nullptr; uint32_t* span4 = nullptr;
  uint32_t* cigar = nullptr; const uint64_t* cigar_off = nullptr; uint32_t* cigar_len = nullptr;
  uint8_t* ops = nullptr; const uint64_t* ops_off = nullptr; uint32_t* ops_len = nullptr;
  PackedCigars* packed = nullptr;                        // the run-length CIGARs as one dense array (replaces cigar / cigar_off / cigar_len)
  const std::function<int()>* while_running = nullptr;  // host work to do between the launch and the wait
  WfaOnDevice* on_device = nullptr;                      // run-length CIGARs are produced but stay on the device
};
// trgt_wfa_batch proper
int wfa_batch_impl(trgt_hip_ctx* c, const trgt_wfa_params* p, const WfaBatchIO& io);

}  // namespace trgt
