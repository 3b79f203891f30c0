// trgt_amd/csrc/hmm_trace_ppl.hpp -- the trace-back of short alleles whose back-pointers the position-per-lane fill wrote in packed rows
// (hmm_fill_ppl_kernel<G, true>, hmm_ppl.hpp), G = 8 / 16 lanes per allele: 64 / G alleles per wave, like the fill in front of it.
// Included by hmm.hip behind hmm_ppl.hpp; the chase and the decoding are the functions of hmm_traceback.hpp.
//
// What hmm_viterbi_kernel<32, true> does for such a job -- counts cleared, the walk, purity, the path to the front, the visits
// decoded -- and nothing of its fill: no score columns, no transition or emission tables, and a slot of LDS carved for the trace-back
// alone (hmm_trace_ppl_lds.hpp: 2.0 / 2.5 KB per job of a 32-state model instead of 5.5 KB).
//
// A round notes G steps (REC = G): hmm_decode_steps works with one lane per step inside the job's lanes -- its shifts, ballots and
// butterfly stay inside the group.  The other choice, 32 steps noted and decoded in 32 / G passes, needs the carries between steps
// (the state walked before, the last block end) handed from pass to pass through LDS; it was not built.
//
// No group leaves the wave: a group without a job of this width, with an allele of no bases or with a long allele handed to
// hmm_traceback_long_kernel only skips the predicated body below.
#pragma once

#include "hmm_trace_ppl_lds.hpp"
static_assert(HMM_TP_CODE_PAD == HMM_CODE_PAD, "the window of symbol codes reaches as far behind the staged columns as hmm_trace_rounds fills it");
static_assert(HMM_TP_COLS + 2 <= HMM_CODE_WINDOW, "a chunk's symbol codes fit the window");

// What a launch gets (the buffers of HmmLaunchBufs, the class's list and its slot sizes)
struct HmmTracePplArgs {
  const HmmJobDev* jobs; const HmmSetDev* sets; const uint8_t* model; const uint8_t* seq_blob; const uint8_t* bp_ws; uint32_t* visit_ws;
  uint16_t* path; uint32_t* path_len; int32_t* spans3; uint32_t* n_spans; uint32_t* counts; double* purity; int32_t* edit_out; int32_t* maxd_out;
  uint32_t n_launch_jobs;         // jobs of the list (a device-resolved list: at most) ...
  const uint32_t* n_jobs_dev;     // ... and where the device counted them (else null)
  uint32_t lds_per_job[2];        // hmm_trace_ppl_lds(8 | 16, largest model of the class).total
  int long_min;                   // columns from which an allele goes to hmm_traceback_long_kernel ...
  uint32_t* long_list;            // ... through this list (null: none can be that long)
  uint32_t n_blocks8;             // hmm_trace_ppl_both_kernel: its first workgroups take the jobs of 8 lanes
};

// the jobs [64 / G * block, 64 / G * (block + 1)) of the list that have fill width G
template <int G>
__device__ __forceinline__ void hmm_trace_ppl_wave(const HmmTracePplArgs& a, const uint32_t block) {
  const HmmJobDev* __restrict__ jobs = a.jobs; const HmmSetDev* __restrict__ sets = a.sets;
  const uint8_t* __restrict__ model = a.model; const uint8_t* __restrict__ seq_blob = a.seq_blob; const uint8_t* __restrict__ bp_ws = a.bp_ws;
  uint32_t* __restrict__ visit_ws = a.visit_ws; uint16_t* __restrict__ path = a.path; uint32_t* __restrict__ path_len = a.path_len;
  int32_t* __restrict__ spans3 = a.spans3; uint32_t* __restrict__ n_spans = a.n_spans; uint32_t* __restrict__ counts = a.counts;
  double* __restrict__ purity = a.purity; int32_t* __restrict__ edit_out = a.edit_out; int32_t* __restrict__ maxd_out = a.maxd_out;
  uint32_t n_launch_jobs = a.n_launch_jobs;
  const uint32_t* __restrict__ n_jobs_dev = a.n_jobs_dev; uint32_t* __restrict__ long_list = a.long_list;
  const uint32_t lds_per_job = a.lds_per_job[G == 8 ? 0 : 1];
  const int long_min = a.long_min;
  static_assert(G == 8 || G == 16, "jobs of 8 or 16 lanes");
  extern __shared__ __align__(16) unsigned char lds_all[];
  constexpr int JPW = 64 / G;
  if (n_jobs_dev) n_launch_jobs = *n_jobs_dev;  // a job list resolved on the device (hmm_resolve_kernel): the grid covers all candidates
  const int hw = (int)threadIdx.x, grp = hw / G, tid = hw % G;
  const uint32_t jidx = block * (uint32_t)JPW + (uint32_t)grp;
  bool live = jidx < n_launch_jobs;
  HmmJobDev job{}; HmmSetDev set{};
  set.S = 8; set.n_blocks = 1;
  if (live) {
    job = jobs[jidx];
    set = sets[job.set];
    live = hmm_ppl_group(set.ppl_lanes) == G;  // (a class with both widths: the list is walked once per width)
  }
  const int S = (int)set.S, nb = (int)set.n_blocks, n_motifs = nb - 1;
  const int qlen = (int)job.seq_len, L = qlen + 2;
  if (live) {
    for (int m = tid; m < n_motifs; m += G) counts[job.count_off + m] = 0;
    if (qlen == 0) {  // Hmm::label returns an empty path; calc_purity returns NaN (hmm_model.rs:145-147, purity.rs:7-9)
      if (tid == 0) {
        if (path_len) path_len[job.job_index] = 0;
        n_spans[job.job_index] = 0;
        purity[job.job_index] = __builtin_nan("");
        if (edit_out) edit_out[job.job_index] = 0;
        if (maxd_out) maxd_out[job.job_index] = 0;
      }
      live = false;
    } else if (long_list && job.map_off && L >= long_min) {  // long alleles are traced back by hmm_traceback_long_kernel, behind this launch on the same stream
      if (tid == 0) long_list[1 + atomicAdd(long_list, 1u)] = jidx;
      live = false;
    }
  }
  if (live) {
    // ---- LDS of my job: the slot is the class's, the carve-up my own set's
    unsigned char* const lds = lds_all + (size_t)grp * lds_per_job;
    const HmmTracePplLds lay = hmm_trace_ppl_lds(G, S, nb);
    int* const tb = reinterpret_cast<int*>(lds + lay.tb);
    uint32_t* const l_inst = reinterpret_cast<uint32_t*>(lds + lay.inst);
    uint32_t* const l_info = reinterpret_cast<uint32_t*>(lds + lay.info);
    uint32_t* const l_blocks = reinterpret_cast<uint32_t*>(lds + lay.blocks);
    uint8_t* const l_flags = lds + lay.flags;
    uint8_t* const l_mot = lds + lay.mot;
    uint32_t* const l_cnt = reinterpret_cast<uint32_t*>(lds + lay.cnt);
    uint32_t* const l_rec = reinterpret_cast<uint32_t*>(lds + lay.rec);
    uint32_t* const l_vis = reinterpret_cast<uint32_t*>(lds + lay.vis);
    uint8_t* const l_seq = lds + lay.seq;
    uint8_t* const l_stage = lds + lay.stage;
    const uint16_t* g_inst = reinterpret_cast<const uint16_t*>(model + set.off_inst);
    const int16_t* g_block = reinterpret_cast<const int16_t*>(model + set.off_block);
    const uint32_t* g_blocks = reinterpret_cast<const uint32_t*>(model + set.off_blocks);
    const uint8_t* g_flags = model + set.off_flags;
    const uint8_t* g_motifs = model + set.off_motifs;
    const int mot_bytes = (S - 7 - n_motifs) / 3;
    const HmmSyncN sync{64};  // one wave: fences
    // The set's tables in two steps.  First every global load a lane needs, into registers: a fixed number per lane (at most
    // HMM_TP_MAX_STATES states and HMM_TP_MAX_BLOCKS blocks: the launcher's condition), none depending on another, so all are in flight
    // at once.  Then, from LDS, what the walk reads.  (hmm_pred_entry straight from global memory is three dependent loads per entry, and
    // with G lanes instead of 32 a job has up to sixteen entries per lane.)
    constexpr int KS = HMM_TP_MAX_STATES / G, KB = 4 * HMM_TP_MAX_BLOCKS / G;
    int16_t* const t_block = reinterpret_cast<int16_t*>(l_stage);  // [S] the block of a state (the staging window is free until the walk begins)
    uint32_t r_inst[KS][4], r_blocks[KB];
    int r_blk[KS];
    uint32_t r_flag[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int st = tid + k * G;
      const bool ok = st < S;
#pragma unroll
      for (int b = 0; b < 4; ++b) r_inst[k][b] = ok ? (uint32_t)g_inst[b * S + st] : 0u;
      r_blk[k] = ok ? (int)g_block[st] : -1;
      r_flag[k] = ok ? (uint32_t)g_flags[st] : 0u;
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) r_blocks[k] = tid + k * G < 4 * nb ? g_blocks[tid + k * G] : 0u;
    const uint32_t r_mot = tid < mot_bytes ? (uint32_t)g_motifs[tid] : 0u;  // (class 0: at most 8 motif bytes)
#pragma unroll
    for (int k = 0; k < KS; ++k)
      if (tid + k * G < S) { l_flags[tid + k * G] = (uint8_t)r_flag[k]; t_block[tid + k * G] = (int16_t)r_blk[k]; }
#pragma unroll
    for (int k = 0; k < KB; ++k) if (tid + k * G < 4 * nb) l_blocks[tid + k * G] = r_blocks[k];
    if (tid < mot_bytes) l_mot[tid] = (uint8_t)r_mot;
    for (int i = tid; i < n_motifs; i += G) l_cnt[i] = 0;
    sync.lds();
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int st = tid + k * G;
      if (st < S) {
        uint4 pe;
        pe.x = hmm_pred_entry(r_inst[k][0], S, nb, l_flags, t_block, l_blocks); pe.y = hmm_pred_entry(r_inst[k][1], S, nb, l_flags, t_block, l_blocks);
        pe.z = hmm_pred_entry(r_inst[k][2], S, nb, l_flags, t_block, l_blocks); pe.w = hmm_pred_entry(r_inst[k][3], S, nb, l_flags, t_block, l_blocks);
        *reinterpret_cast<uint4*>(l_inst + 4 * st) = pe;
        l_info[st] = hmm_state_info(st, r_blk[k], nb, l_blocks, l_mot, r_flag[k]);
      }
    }
    if (tid == 0) { hmm_trace_init(tb, S, L); tb[TB_LOC] = 0; }  // (the end state's back-pointer: a constant 0)
    sync.lds();
    // ---- traceback, fused with the events, the purity counts and the motif-visit collection (hmm_traceback.hpp); rows of G bytes
    const uint8_t* const seq = seq_blob + job.seq_off;
    const uint8_t* const bp = bp_ws + job.bp_off;
    uint16_t* const pbuf = path ? path + job.path_off : nullptr;
    uint32_t* const g_vis = visit_ws + job.visit_off;  // visits HMM_TP_VIS, HMM_TP_VIS + 1, ... at their own index
    const int pcap = (int)job.path_cap;
    const unsigned long long gmask = ((1ull << G) - 1ull) << (grp * G);  // the lanes of my job in this wave
    const HmmTraceLds tl{tb, l_inst, l_info, l_blocks, l_flags, l_stage, l_seq, l_mot, l_vis, l_cnt, l_rec};
    hmm_trace_rounds<G, true, HMM_TP_VIS, HMM_TP_COLS>(sync, tid, G, tl, true, G, HMM_TP_COLS, S, nb, L, seq, bp, g_vis, pbuf, pcap, gmask);
    const int np = tb[TB_NPATH];
    hmm_path_to_front(sync, tid, G, pbuf, np, pcap);
    if (tid == 0) hmm_store_purity(job.job_index, np, tb[TB_EDIT], tb[TB_REF], qlen, path_len, purity, edit_out, maxd_out);
    hmm_decode_visits<HMM_TP_VIS, hmm_trace_ppl_stage_bytes(G)>(sync, tid, G, tl, nb, g_vis, spans3 + 3 * job.span_off, n_spans + job.job_index, counts + job.count_off);
  }
}

template <int G>
__global__ void __launch_bounds__(64) hmm_trace_ppl_kernel(const HmmTracePplArgs a) { hmm_trace_ppl_wave<G>(a, blockIdx.x); }

// A class with sets of both widths: ONE launch, whose first n_blocks8 workgroups walk the list for the jobs of 8 lanes and the others for
// those of 16.  (One launch per width, one behind the other on the class's stream, added up the two longest alleles: each launch lasts
// as long as its longest walk -- the class-0 trace-back of a cfg4 call 0.33 + 0.30 ms against 0.52 ms through hmm_viterbi_kernel.)
__global__ void __launch_bounds__(64) hmm_trace_ppl_both_kernel(const HmmTracePplArgs a) {
  if (blockIdx.x < a.n_blocks8) hmm_trace_ppl_wave<8>(a, blockIdx.x);
  else hmm_trace_ppl_wave<16>(a, blockIdx.x - a.n_blocks8);
}
