// trgt_amd/csrc/hmm_big.hpp -- Viterbi fill and trace-back of LARGE motif-set models (included by hmm.hip behind hmm_viterbi_kernel).
//
// hmm_viterbi_kernel gives a thread to every lane of a model: 1 024 lanes at most (trgt_hmm_batch), 448 in the locus path's launch
// classes.  Here the lanes of a model are tiled over a workgroup of 1 024 threads: lane l belongs to thread l % 1024 as its tile
// l / 1024, so a "virtual wave" (64 consecutive lanes of the set's lane -> state table, layout_set) is still ONE hardware wave, and the
// deletion chains -- which that table keeps in consecutive lanes -- are still walked by DPP shifts; a chain longer than a wave takes
// further rounds through LDS as before (set.chain_rounds).  Per state only the two score columns (16 B) live in LDS during the fill;
// a thread's transition terms and predecessor indices sit in registers (HMM_BIG_TILES tiles), the emission term of the next column is
// fetched from the model tables in global memory (L2) a column ahead.  Back-pointers: one byte per cell in the job's workspace.
//
// The f64 operations are the reference's in the reference's order, as in hmm_viterbi_kernel's four-pass LDS fill, which this is a
// restatement of: (prev + ln p) + emission, the first strict maximum in predecessor order (hmm_model.rs:54-142); silent states in the
// passes chains | run end + run start | block starts (any topological order gives the same values, hmm_model.rs:206-240).
//
// Trace-back: the serial chase of hmm_viterbi_kernel (thread 0 follows the back-pointers through LDS-staged columns, the lanes of the
// first wave decode the noted steps) for alleles of ANY length -- shared code, not a copy: hmm_traceback.hpp, with this kernel's barriers.  The chunk-map kernel (hmm_traceback_long_kernel) walks every chunk
// from every entry state, S * columns step-lanes and 12 S bytes of map per chunk, and its LDS plan (21 B per state + staging + maps)
// does not fit 4 096 states; the serial chase is exact and its measured share of such a job is in DESIGN.md 5.
// The predecessor entries of the chase (16 B per state) take the place of the score columns once the fill is through.
#pragma once

constexpr int HMM_BIG_THREADS = 1024;
constexpr int HMM_BIG_TILES = 4;               // lanes per thread
constexpr uint32_t HMM_BIG_MAX_STATES = 4096;  // = HMM_BIG_THREADS * HMM_BIG_TILES lanes (a model's lanes: its states rounded up to whole waves)
constexpr int HMM_BIG_STAGE_COLS = 8;          // back-pointer columns staged per chunk of the trace-back

struct HmmBigLds { uint32_t sc, info, flags, blocks, stage, seq, mot, vis, cnt, rec, total; };
// (monotone in S and nb: a class's launch is sized by its largest model, every job carves up its own)
__host__ __device__ inline HmmBigLds hmm_big_lds(uint32_t S, uint32_t nb) {
  HmmBigLds l;
  const uint32_t spad = (S + 15u) & ~15u, stage = (uint32_t)HMM_BIG_STAGE_COLS * spad;
  uint32_t o = 64;                                            // trace-back state shared between the walker and the stagers
  l.sc = o; o += 16u * S;                                     // fill: two score columns, f64 [2][S]; trace-back: hmm_pred_entry [S][4]
  l.info = o; o += 4u * S;                                    // [S] the trace-back word of a state
  l.flags = o; o += spad;                                     // [S]
  l.blocks = o; o += 16u * nb;                                // [4][nb]
  l.stage = o; o += stage > (uint32_t)HMM_STAGE_BYTES ? stage : (uint32_t)HMM_STAGE_BYTES;
  l.seq = o; o += HMM_CODE_WINDOW + HMM_CODE_PAD;
  l.mot = o; o += (S / 3u + 15u) & ~15u;
  l.vis = o; o += 12u * HMM_VIS_LDS;
  l.cnt = o; o += (4u * nb + 15u) & ~15u;
  l.rec = o; o += 8u * 64u;
  l.total = o;
  return l;
}

__global__ void __launch_bounds__(HMM_BIG_THREADS) hmm_viterbi_big_kernel(
    const HmmJobDev* __restrict__ jobs, const HmmSetDev* __restrict__ sets, const uint8_t* __restrict__ model, const uint8_t* __restrict__ seq_blob,
    uint8_t* __restrict__ bp_ws, uint32_t* __restrict__ visit_ws, uint16_t* __restrict__ path, uint32_t* __restrict__ path_len,
    int32_t* __restrict__ spans3, uint32_t* __restrict__ n_spans, uint32_t* __restrict__ counts, double* __restrict__ purity,
    int32_t* __restrict__ edit_out, int32_t* __restrict__ maxd_out, uint32_t n_launch_jobs, const uint32_t* __restrict__ n_jobs_dev) {
  extern __shared__ __align__(16) unsigned char lds_big[];
  if (n_jobs_dev) n_launch_jobs = *n_jobs_dev;  // a job list resolved on the device (hmm_resolve_*): the grid covers all candidates
  constexpr int nthr = HMM_BIG_THREADS, K = HMM_BIG_TILES;
  const int tid = (int)threadIdx.x;
  const uint32_t jidx = blockIdx.x;
  if (jidx >= n_launch_jobs) return;
  const HmmJobDev job = jobs[jidx];
  const HmmSetDev set = sets[job.set];
  const int S = (int)set.S, nb = (int)set.n_blocks, n_motifs = nb - 1;
  const int qlen = (int)job.seq_len, L = qlen + 2;
  const int Spad = (S + 15) & ~15;
  const double NINF = -__builtin_huge_val();

  HP_DECL;
  for (int m = tid; m < n_motifs; m += nthr) counts[job.count_off + m] = 0;
  if (qlen == 0) {  // Hmm::label returns an empty path; calc_purity returns NaN (hmm_model.rs:145-147, purity.rs:7-9)
    if (tid == 0) {
      if (path_len) path_len[job.job_index] = 0;
      n_spans[job.job_index] = 0;
      purity[job.job_index] = __builtin_nan("");
      if (edit_out) edit_out[job.job_index] = 0;
      if (maxd_out) maxd_out[job.job_index] = 0;
    }
    return;
  }
  const HmmBigLds lay = hmm_big_lds((uint32_t)S, (uint32_t)nb);
  int* tb = reinterpret_cast<int*>(lds_big);
  int& l_bp_rs = tb[12];  // (behind the words TB_* of the trace-back)
  double* sc0 = reinterpret_cast<double*>(lds_big + lay.sc);
  double* sc1 = sc0 + S;
  uint32_t* l_inst = reinterpret_cast<uint32_t*>(lds_big + lay.sc);  // (behind the fill)
  uint32_t* l_info = reinterpret_cast<uint32_t*>(lds_big + lay.info);
  uint8_t* l_flags = lds_big + lay.flags;
  uint32_t* l_blocks = reinterpret_cast<uint32_t*>(lds_big + lay.blocks);
  uint8_t* l_stage = lds_big + lay.stage;
  uint8_t* l_seq = lds_big + lay.seq;
  uint8_t* l_mot = lds_big + lay.mot;
  uint32_t* l_vis = reinterpret_cast<uint32_t*>(lds_big + lay.vis);
  uint32_t* l_cnt = reinterpret_cast<uint32_t*>(lds_big + lay.cnt);
  uint32_t* l_rec = reinterpret_cast<uint32_t*>(lds_big + lay.rec);

  const double* g_inlp = reinterpret_cast<const double*>(model + set.off_inlp);
  const double* g_em = reinterpret_cast<const double*>(model + set.off_em);
  const uint16_t* g_inst = reinterpret_cast<const uint16_t*>(model + set.off_inst);
  const int16_t* g_block = reinterpret_cast<const int16_t*>(model + set.off_block);
  const uint32_t* g_blocks = reinterpret_cast<const uint32_t*>(model + set.off_blocks);
  const uint8_t* g_flags = model + set.off_flags;
  const uint8_t* g_motifs = model + set.off_motifs;
  const uint16_t* g_perm = reinterpret_cast<const uint16_t*>(model + set.off_perm);
  const int mot_bytes = (S - 7 - n_motifs) / 3;
  for (int i = tid; i < mot_bytes; i += nthr) l_mot[i] = g_motifs[i];
  for (int i = tid; i < n_motifs; i += nthr) l_cnt[i] = 0;
  for (int i = tid; i < S; i += nthr) l_flags[i] = g_flags[i];
  for (int i = tid; i < 4 * nb; i += nthr) l_blocks[i] = g_blocks[i];
  __syncthreads();
  // traceback word of a state: kind (0 outside any block, 1 block start, 2 block end, 3 skip state, 4 match, 5 insertion, 6 deletion)
  // | emits << 3 | block << 8 | expected motif base << 16 (match states) -- as in hmm_viterbi_kernel
  for (int st = tid; st < S; st += nthr) {
    const int blk = (int)g_block[st];
    uint32_t kind = 0, expected = 0;
    if (blk >= 0) {
      const int bstart = (int)l_blocks[0 * nb + blk], bend = (int)l_blocks[1 * nb + blk];
      if (st == bstart) kind = 1;
      else if (st == bend) kind = 2;
      else if (blk == nb - 1) kind = 3;
      else {
        const int mlen = (int)l_blocks[2 * nb + blk], off = st - bstart - 1, k = off / mlen;
        kind = 4u + (uint32_t)k;
        if (k == 0) expected = l_mot[l_blocks[3 * nb + blk] + off];
      }
    }
    l_info[st] = kind | ((uint32_t)(l_flags[st] & 1) << 3) | ((uint32_t)(blk & 0xFF) << 8) | (expected << 16);
  }

  // ---- my lanes' states and their tables, in registers
  int t_st[K], t_nin[K], t_q[K][4], t_ridx[K];
  bool t_act[K], t_emit[K], t_del[K], t_end[K], t_start[K], t_chain[K], t_xwave[K];
  double t_lp[K][4];
  bool t_step[K];  // takes the lane before it in the chain walk (else its transition term there is -inf)
  const int NL = (int)set.n_lanes;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int lane = tid + nthr * j;
    const int stl = lane < NL ? (int)g_perm[lane] : 0xFFFF;
    const bool act = stl < S;
    const int st = act ? stl : 0;
    const int n_in = (int)model[set.off_nin + st], level = (int)model[set.off_level + st];
    t_st[j] = st; t_act[j] = act; t_nin[j] = n_in; t_emit[j] = act && level == 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      t_lp[j][b] = g_inlp[(size_t)b * S + st];
      t_q[j][b] = (n_in != 0xFF && n_in > b) ? (int)g_inst[(size_t)b * S + st] : 0;  // slots that do not exist read state 0 and are ignored (n_in guards the comparison)
    }
    const int blk = act ? (int)g_block[st] : -1;
    const int b_ms = blk >= 0 ? (int)l_blocks[0 * nb + blk] : -1, b_me = blk >= 0 ? (int)l_blocks[1 * nb + blk] : -1, b_n = blk >= 0 ? (int)l_blocks[2 * nb + blk] : 0;
    t_end[j] = act && blk >= 0 && st == b_me;
    t_start[j] = act && blk >= 0 && st == b_ms;
    t_del[j] = act && level > 0 && !t_end[j] && !t_start[j] && n_in != 0xFF && blk >= 0;
    t_chain[j] = t_del[j] || t_end[j];
    // a chain state's LAST predecessor is the state before it = the lane before it (or the last lane of the wave before)
    const bool chain_prev = t_del[j] ? n_in > 1 : t_end[j] ? n_in > 2 : false;
    t_xwave[j] = chain_prev && (lane & 63) == 0;
    t_step[j] = chain_prev && !t_xwave[j];
    // the round in which the state is final: the waves between the first lane of its chain (states me - (n - 1) .. me in
    // consecutive lanes) and its own; chain states without a chain (motifs of one base, the skip block's end): round 0
    int ridx = -1;
    if (t_chain[j]) {
      ridx = 0;
      if (b_n > 1 && blk != nb - 1) { const int lane0 = lane - (st - (b_me - (b_n - 1))); ridx = (lane >> 6) - (lane0 >> 6); }
    }
    t_ridx[j] = ridx;
  }
  const int chain_steps = min(63, (int)set.max_mlen - 1);
  const int chain_rounds = (int)set.chain_rounds;
  const double lp_rs0 = g_inlp[1], lp_rs1 = g_inlp[S + 1];  // transition terms of the run start (state 1), evaluated by the run-end thread
  const uint8_t* __restrict__ seq = seq_blob + job.seq_off;
  uint8_t* __restrict__ bp = bp_ws + job.bp_off;
  int win0 = 0;
  auto code_at = [&](int i) -> int { return (int)l_seq[i - win0]; };
  const HmmSyncBlock sync;  // (sync.lds(): not vmcnt -- the back-pointer stores are read again behind a full barrier only)
  __syncthreads();
  HP_MARK(0);

  // ---- Viterbi fill (generate_mats, hmm_model.rs:99-114)
  {
    double* prev = sc0;
    double* cur = sc1;
    double em_next[K];
    uint8_t* __restrict__ bp_col = bp;
    for (int i = 0; i < L; ++i) {
      if ((i % HMM_CODE_WINDOW) == 0) {  // next window of symbol codes (one column more than the window: the look-ahead below)
        sync.lds();
        win0 = i;
        for (int k = tid; k < HMM_CODE_WINDOW + 1 && i + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, i + k, L);
        sync.lds();
        const int sym = code_at(i);
#pragma unroll
        for (int j = 0; j < K; ++j) em_next[j] = t_emit[j] ? g_em[(size_t)sym * S + t_st[j]] : NINF;
      }
      double em[K], best[K];
      int bpi[K];
#pragma unroll
      for (int j = 0; j < K; ++j) em[j] = em_next[j];
      if (i + 1 < L) {  // (the next column's emission terms: their round trip to L2 is off this column's critical path)
        const int sym1 = code_at(i + 1);
#pragma unroll
        for (int j = 0; j < K; ++j) if (t_emit[j]) em_next[j] = g_em[(size_t)sym1 * S + t_st[j]];
      }
      // -- emitting states
#pragma unroll
      for (int j = 0; j < K; ++j) {
        best[j] = NINF; bpi[j] = 0xFF;
        if (t_emit[j]) {
          const int n_in = t_nin[j];
          if (i == 0) {
            if (n_in == 0 && em[j] > NINF) { best[j] = em[j]; bpi[j] = 0xFE; }  // the start state (hmm_model.rs:91-94)
          } else {
            const double s0 = prev[t_q[j][0]], s1 = prev[t_q[j][1]], s2 = prev[t_q[j][2]], s3 = prev[t_q[j][3]];
            const double v0 = (s0 + t_lp[j][0]) + em[j], v1 = (s1 + t_lp[j][1]) + em[j], v2 = (s2 + t_lp[j][2]) + em[j], v3 = (s3 + t_lp[j][3]) + em[j];
            if (n_in > 0 && v0 > best[j]) { best[j] = v0; bpi[j] = 0; }
            if (n_in > 1 && v1 > best[j]) { best[j] = v1; bpi[j] = 1; }
            if (n_in > 2 && v2 > best[j]) { best[j] = v2; bpi[j] = 2; }
            if (n_in > 3 && v3 > best[j]) { best[j] = v3; bpi[j] = 3; }
          }
          cur[t_st[j]] = best[j];
        }
      }
      sync.lds();
      // -- the chains d0 <- d1 <- ... <- block end of all motif blocks: what the other predecessors give, then the walk across the
      //    lanes of a wave (see hmm_viterbi_kernel).  Round r makes the states r waves behind the first lane of their chain final;
      //    a wave runs the rounds in which some lane of it becomes final (a state that is final already is recomputed from the
      //    same final inputs, one that is not yet is overwritten in its own round).  A wave that runs round r also recomputes
      //    its lanes of later rounds and writes those throw-away values to cur[], where the first lane of the next wave may read
      //    them in the same round with no barrier in between: harmless, because what that lane makes of them is thrown away as
      //    well -- its own round comes after the barrier behind the round that made its predecessor final, and no wave writes
      //    a state again after that round except with the identical bits.
      double own[K];
      int own_bp[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (t_chain[j]) {
          const int n_in = t_nin[j];
          const double s0 = cur[t_q[j][0]], s1 = cur[t_q[j][1]];
          const double v0 = (s0 + t_lp[j][0]), v1 = (s1 + t_lp[j][1]);
          if (n_in > 0 && v0 > best[j]) { best[j] = v0; bpi[j] = 0; }
          if (t_end[j] && n_in > 1 && v1 > best[j]) { best[j] = v1; bpi[j] = 1; }
        }
        own[j] = best[j]; own_bp[j] = bpi[j];
      }
      for (int r = 0; r < chain_rounds; ++r) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (__ballot(t_ridx[j] == r) == 0ull) continue;  // (wave-uniform)
          const int chain_bp = t_del[j] ? 1 : 2;
          const double lp_chain = t_del[j] ? t_lp[j][1] : t_lp[j][2], lp_step = t_step[j] ? lp_chain : NINF;
          double b = own[j];
          int bb = own_bp[j];
          if (t_xwave[j]) {  // the state before sits in the wave before: final after the round before
            const double c0 = (cur[t_st[j] - 1] + lp_chain);
            if (c0 > b) { b = c0; bb = chain_bp; }
          }
          double val = b, cand = NINF;
          for (int t = 0; t < chain_steps; ++t) {
            cand = (wave_shr1_f64(val) + lp_step);
            val = max_f64(cand, b);
          }
          if (cand > b) bb = chain_bp;  // (never for the lanes whose transition term is -inf)
          if (t_chain[j]) cur[t_st[j]] = val;
          best[j] = val; bpi[j] = bb;
        }
        if (r + 1 < chain_rounds) sync.lds();
      }
      sync.lds();
      // -- run end: the block ends in block order; then the run start {start state, run end}
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (t_act[j] && t_nin[j] == 0xFF) {
          const double start_now = cur[0];
          double re = NINF; int re_bp = 0xFF;
          for (int b = 0; b < nb; ++b) {
            const double v = (cur[l_blocks[1 * nb + b]] + t_lp[j][0]);
            if (v > re) { re = v; re_bp = b; }
          }
          cur[t_st[j]] = re; best[j] = re; bpi[j] = re_bp;
          double br = NINF; int pr = 0xFF;
          const double v0 = (start_now + lp_rs0), v1 = (re + lp_rs1);
          if (v0 > br) { br = v0; pr = 0; }
          if (v1 > br) { br = v1; pr = 1; }
          cur[1] = br; l_bp_rs = pr;
        }
      }
      sync.lds();
      // -- block starts: {run start, own block end}
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (t_start[j]) {
          const int n_in = t_nin[j];
          const double s0 = cur[t_q[j][0]], s1 = cur[t_q[j][1]];
          const double v0 = (s0 + t_lp[j][0]), v1 = (s1 + t_lp[j][1]);
          if (n_in > 0 && v0 > best[j]) { best[j] = v0; bpi[j] = 0; }
          if (n_in > 1 && v1 > best[j]) { best[j] = v1; bpi[j] = 1; }
          cur[t_st[j]] = best[j];
        }
      }
      sync.lds();
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (t_act[j]) {
          if (t_st[j] == 1) bpi[j] = l_bp_rs;  // the run start was evaluated by the run-end thread
          bp_col[t_st[j]] = (uint8_t)bpi[j];
        }
      }
      bp_col += Spad;
      double* t = prev; prev = cur; cur = t;
    }
  }
  __syncthreads();  // the back-pointer columns written by all waves are read back from here on; the score columns are free
  HP_MARK(1);
  // (bit 15 of a predecessor entry: that state emits a base -- the trace-back then knows it on arrival, without a look-up of its own)
  for (int i = tid; i < 4 * S; i += nthr) l_inst[4 * (i % S) + i / S] = hmm_pred_entry(g_inst[i], S, nb, g_flags, g_block, g_blocks);
  if (tid == 0) hmm_trace_init(tb, S, L);
  __syncthreads();

  // ---- traceback: the serial chase of hmm_viterbi_kernel (hmm_traceback.hpp) over rows of one byte per state, thread 0 chases, the
  //      lanes of wave 0 decode 64 noted steps at a time
  uint16_t* pbuf = path ? path + job.path_off : nullptr;
  uint32_t* const g_vis = visit_ws + job.visit_off;  // visits HMM_VIS_LDS, HMM_VIS_LDS + 1, ... at their own index
  const int pcap = (int)job.path_cap;
  const HmmTraceLds tl{tb, l_inst, l_info, l_blocks, l_flags, l_stage, l_seq, l_mot, l_vis, l_cnt, l_rec};
  hmm_trace_rounds<64, false>(sync, tid, nthr, tl, false, Spad, HMM_BIG_STAGE_COLS, S, nb, L, seq, bp, g_vis, pbuf, pcap, ~0ull);
  const int np = tb[TB_NPATH];
  HP_MARK(2);
  hmm_path_to_front(sync, tid, nthr, pbuf, np, pcap);
  if (tid == 0) hmm_store_purity(job.job_index, np, tb[TB_EDIT], tb[TB_REF], qlen, path_len, purity, edit_out, maxd_out);
  hmm_decode_visits(sync, tid, nthr, tl, nb, g_vis, spans3 + 3 * job.span_off, n_spans + job.job_index, counts + job.count_off);
  HP_MARK(3);
}
