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
// first wave decode the noted steps) for alleles of ANY length.  The chunk-map kernel (hmm_traceback_long_kernel) walks every chunk
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
  int &tb_state = tb[0], &tb_idx = tb[1], &tb_done = tb[2], &tb_npath = tb[3], &tb_nvisit = tb[4], &tb_edit = tb[5],
      &tb_ref = tb[6], &tb_next = tb[7], &tb_vb1 = tb[8], &tb_nrec = tb[9], &tb_more = tb[10], &l_bp_rs = tb[12];
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
  auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };  // (not vmcnt: the back-pointer stores are read again behind a full barrier only)
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
        lds_barrier();
        win0 = i;
        for (int k = tid; k < HMM_CODE_WINDOW + 1 && i + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, i + k, L);
        lds_barrier();
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
      lds_barrier();
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
        if (r + 1 < chain_rounds) lds_barrier();
      }
      lds_barrier();
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
      lds_barrier();
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
      lds_barrier();
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
  if (tid == 0) {
    tb_state = S - 1; tb_idx = L - 1; tb_done = 0; tb_npath = 0; tb_nvisit = 0; tb_edit = 0; tb_ref = 0; tb_next = -1; tb_vb1 = 0;
  }
  __syncthreads();

  // ---- traceback (hmm_model.rs:125-142) fused with get_events/calc_purity (events.rs:17-86, purity.rs:6-41) and motif-visit
  //      collection (operations.rs:26-40): the round loop of hmm_viterbi_kernel (rows of one byte per state), thread 0 chases,
  //      the lanes of wave 0 decode HMM_REC noted steps at a time
  const int rstride = Spad;
  const int cols_per_chunk = HMM_BIG_STAGE_COLS;
  uint16_t* pbuf = path ? path + job.path_off : nullptr;
  uint32_t* const g_vis = visit_ws + job.visit_off;  // visits HMM_VIS_LDS, HMM_VIS_LDS + 1, ... at their own index
  const int pcap = (int)job.path_cap;
  constexpr int HMM_REC = 64;
  const int hwlane = tid & 63;
  const unsigned long long below = (1ull << hwlane) - 1ull;
  while (true) {
    if (tb_done) break;
    const int c1 = tb_idx + 1, c0 = max(0, c1 - cols_per_chunk);
    {
      const uint4* src = reinterpret_cast<const uint4*>(bp + (size_t)c0 * rstride);
      uint4* dst = reinterpret_cast<uint4*>(l_stage);
      const int n16 = ((c1 - c0) * rstride + 15) / 16;
      for (int i = tid; i < n16; i += nthr) dst[i] = src[i];
      // ... and the symbol codes of the same columns, plus those a motif copy starting in the last of them reaches into
      win0 = c0;
      for (int k = tid; k < c1 - c0 + HMM_CODE_PAD && c0 + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, c0 + k, L);
    }
    lds_barrier();
    for (;;) {
      if (tid == 0) {  // ---- the chase
        int state = tb_state, idx = tb_idx, n = 0;
        int row = (idx - c0) * rstride;  // offset of column idx in the staged chunk
        int emits = (int)((l_info[state] >> 3) & 1u);
        while (state != 0 && idx >= c0 && n < HMM_REC) {
          l_rec[2 * n] = (uint32_t)state; l_rec[2 * n + 1] = (uint32_t)idx; ++n;
          const uint4 pred4 = *reinterpret_cast<const uint4*>(l_inst + 4 * state);  // all four predecessors: no second round trip behind b
          const int b = l_stage[row + state];
          uint32_t pe = (b & 2) ? ((b & 1) ? pred4.w : pred4.z) : ((b & 1) ? pred4.y : pred4.x);  // predecessor | its "emits" bit << 15
          if (state == S - 2) { const uint32_t be_ = l_blocks[1 * nb + (b < nb ? b : 0)]; pe = be_ | ((uint32_t)(l_flags[be_] & 1) << 15); }  // the run end: from a block end
          if (emits) { --idx; row -= rstride; }
          emits = (int)((pe >> 15) & 1u);
          state = (int)(pe & 0x7FFFu);
        }
        tb_state = state; tb_idx = idx; tb_nrec = n;
        tb_more = state == 0 ? 2 : (idx >= c0 ? 1 : 0);
      }
      lds_barrier();
      const int more = tb_more;  // (read before the next barrier: thread 0 writes it again right behind that one)
      if (tid < HMM_REC) {  // ---- what the noted steps mean (events.rs:17-86, purity.rs:6-41, operations.rs:26-57), one lane per step
        const int n = tb_nrec, np0 = tb_npath, nv0 = tb_nvisit, nxt0 = tb_next, vb0 = tb_vb1;
        const bool valid = tid < n;
        const int state = valid ? (int)l_rec[2 * tid] : 0, idx = valid ? (int)l_rec[2 * tid + 1] : 0;
        const uint32_t inf = valid ? l_info[state] : 0u;
        const int kind = (int)(inf & 7u), blk = (int)((inf >> 8) & 0xFFu), expected = (int)((inf >> 16) & 0xFFu);
        if (valid && pbuf && np0 + tid < pcap) pbuf[pcap - 1 - (np0 + tid)] = (uint16_t)state;
        // the state walked just before this one (the step before: the lane before)
        const int up = __shfl_up(state, 1);
        const int nxt = tid == 0 ? nxt0 : up;
        // MotifStart (1) adds the implied leading deletions, Skip (3) / Mismatch / Ins (5) / Del (6) are edits, Skip / Match-state /
        // Del consume a reference base
        const int qbase = valid ? hmm_code_char(code_at(idx)) : 0;
        const int dels = kind == 1 ? nxt - state - 1 : 0;
        const int mism = kind == 4 && !(qbase == expected || expected == 'N');  // events.rs:66-73
        int edit = valid ? dels + (kind == 3) + mism + (kind == 5) + (kind == 6) : 0;
        int ref = valid ? dels + (kind == 3) + (kind == 4) + (kind == 6) : 0;
        // the last block end (2) walked before this step: the bases of the visit a block start (1) closes are query[idx .. vb1)
        const unsigned long long ends = __ballot(valid && kind == 2), starts = __ballot(valid && kind == 1);
        const unsigned long long ends_below = ends & below;
        const int src_end = ends_below ? 63 - (int)__builtin_clzll(ends_below) : hwlane;
        const int idx_end = __shfl(idx, src_end);
        const int vb1 = ends_below ? idx_end : vb0;
        if (valid && kind == 1) {  // a motif visit
          // remove_imperfect_motifs(.., 6) (operations.rs:45-57): only copies of STR motifs can be dropped -- short ones, and ones
          // whose bases differ from the motif (its bases are columns idx + 1 .. idx + mlen: in the window)
          uint32_t drop = 0;
          const int mlen = (int)l_blocks[2 * nb + blk];
          if (blk != nb - 1 && mlen <= 6) {
            if (vb1 - idx < mlen) drop = 1;
            else {
              const uint8_t* mot = l_mot + l_blocks[3 * nb + blk];
              for (int jj = 0; jj < mlen; ++jj) {
                const int obs = hmm_code_char(code_at(idx + jj + 1));
                if (mot[jj] != 'N' && obs != mot[jj]) drop = 1;
              }
            }
          }
          const int nv = nv0 + (int)__builtin_popcountll(starts & below);
          uint32_t* vrec = nv < HMM_VIS_LDS ? l_vis + 3 * nv : g_vis + 3 * (size_t)nv;
          vrec[0] = (uint32_t)blk | (drop << 15); vrec[1] = (uint32_t)idx; vrec[2] = (uint32_t)vb1;
        }
        // sums over the round (butterfly inside the wave)
#pragma unroll
        for (int o = HMM_REC / 2; o >= 1; o >>= 1) { edit += __shfl_xor(edit, o); ref += __shfl_xor(ref, o); }
        const int src_last_end = ends ? 63 - (int)__builtin_clzll(ends) : hwlane;
        const int idx_last_end = __shfl(idx, src_last_end);
        const int last_state = __shfl(state, max(n - 1, 0));
        if (tid == 0) {
          int np = np0 + n;
          if (more == 2) { if (pbuf && np < pcap) pbuf[pcap - 1 - np] = 0; ++np; tb_done = 1; }
          tb_npath = np; tb_nvisit = nv0 + (int)__builtin_popcountll(starts); tb_edit += edit; tb_ref += ref;
          if (n > 0) tb_next = last_state;
          if (ends) tb_vb1 = idx_last_end;
        }
      }
      lds_barrier();
      if (more != 1) break;
    }
  }
  const int np = tb_npath;
  HP_MARK(2);
  // ---- state path: shift the reversed tail to the front (forward order)
  if (pbuf) {
    const int n = min(np, pcap), shift = pcap - n;
    __syncthreads();  // (the path was written by wave 0)
    for (int base = 0; base < n; base += nthr) {
      const int f = base + tid;
      uint16_t v = 0;
      if (f < n) v = pbuf[shift + f];
      __syncthreads();
      if (f < n) pbuf[f] = v;
      __syncthreads();
    }
  }
  // ---- decode (thread 0): purity, label_motifs over the kept copies, skip filter, counts, collapse.  Visits were recorded back to
  //      front: the last ones recorded (the first of the allele) sit in global memory and come through LDS in chunks.
  int ns = 0, cum = 0, last_motif = -1, last_end = -1;
  int32_t* const sp = spans3 + 3 * job.span_off;
  auto take_visit = [&](const uint32_t* vrec) {
    const int blk = (int)(vrec[0] & 0x7FFFu), b0 = (int)vrec[1], b1 = (int)vrec[2];
    const bool keep = (vrec[0] >> 15) == 0;
    const int cnt = b1 - b0;
    const int start = cum, end = cum + cnt;
    cum = end;
    const int motif = keep ? blk : nb - 1;
    if (motif < n_motifs) {
      l_cnt[motif] += 1;
      if (ns > 0 && last_motif == motif && last_end == start) { sp[3 * (ns - 1) + 2] = end; }
      else { sp[3 * ns + 0] = motif; sp[3 * ns + 1] = start; sp[3 * ns + 2] = end; ++ns; last_motif = motif; }
      last_end = end;
    }
  };
  if (tid == 0) {
    if (path_len) path_len[job.job_index] = (uint32_t)np;
    const int edit = tb_edit, mx = max(tb_ref, qlen);
    purity[job.job_index] = ((double)mx - (double)edit) / (double)mx;
    if (edit_out) edit_out[job.job_index] = edit;
    if (maxd_out) maxd_out[job.job_index] = mx;
  }
  int v = tb_nvisit - 1;
  constexpr int VIS_CHUNK = HMM_STAGE_BYTES / 12;
  uint32_t* const l_vchunk = reinterpret_cast<uint32_t*>(l_stage);  // (the staging window of the back-pointers is free now)
  while (v >= HMM_VIS_LDS) {
    const int n = min(v - HMM_VIS_LDS + 1, VIS_CHUNK), v0 = v - n + 1;
    __syncthreads();  // (the visits were written by wave 0; the chunk before has been consumed)
    for (int k = tid; k < 3 * n; k += nthr) l_vchunk[k] = g_vis[3 * (size_t)v0 + k];
    lds_barrier();
    if (tid == 0) for (int k = n - 1; k >= 0; --k) take_visit(l_vchunk + 3 * k);
    v -= n;
  }
  if (tid == 0) {
    for (; v >= 0; --v) take_visit(l_vis + 3 * v);
    n_spans[job.job_index] = (uint32_t)ns;
  }
  lds_barrier();
  for (int m = tid; m < n_motifs; m += nthr) counts[job.count_off + m] = l_cnt[m];
  HP_MARK(3);
}
