// trgt_amd/csrc/hmm_traceback.hpp -- the trace-back code shared by hmm_viterbi_kernel, hmm_trace_ppl_kernel (hmm_trace_ppl.hpp),
// hmm_viterbi_big_kernel (hmm_big.hpp) and hmm_traceback_long_kernel (included by hmm.hip ahead of the kernels; everything here is
// inlined into them).
//
// hmm_decode_steps   what up to REC noted steps of the walk mean, one lane per step: all three kernels
// hmm_path_to_front, hmm_store_purity   the end of a job's trace-back: all three kernels
// hmm_trace_rounds, hmm_decode_visits   the serial chase (thread 0 follows the back-pointers through LDS-staged columns, the lanes of
//                    the job's first wave decode the noted steps) and the decode of the motif visits by thread 0: the two fill kernels
//                    and hmm_trace_ppl_kernel, whose "threads" are the G lanes of a job's group.
//                    (The long kernel chases on wave-uniform values and decodes the visits on all its threads.)
#pragma once

// The barriers of a kernel's trace-back.  lds(): LDS traffic only; mem(): the workgroup's global stores are visible afterwards as
// well.  Which barrier is which kind is part of the measured cost of a column: the callers choose, nothing here swaps them.
struct HmmSyncN {  // hmm_viterbi_kernel: a single wave (n == 64) needs a fence only (hmm_sync)
  int n;
  __device__ __forceinline__ void lds() const { hmm_sync(n); }
  __device__ __forceinline__ void mem() const { hmm_sync_mem(n); }
};
struct HmmSyncBlock {  // workgroups of many waves
  __device__ __forceinline__ void lds() const { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }  // (not vmcnt: the back-pointer stores are read again behind a full barrier only)
  __device__ __forceinline__ void mem() const { __syncthreads(); }
};

// What a round of steps takes over from the rounds before it, and what it hands on
struct HmmStepCarry { int np, nv, nxt, vb; };  // path steps so far, visits so far, the state walked before, the column of the last block end
struct HmmStepSums { int edit, ref, n_starts, last_state, idx_last_end; bool any_end; };

// ---- what the noted steps mean (events.rs:17-86, purity.rs:6-41, operations.rs:26-57), one lane per step.  slot: the lane's place among
// the REC lanes of its job (REC = 32: two jobs per wave, gmask: the lanes of mine); n: steps noted in l_rec ([.][2] state, column);
// code_at(i): symbol code of column i; vis_at(nv): where visit record nv goes.  Every lane of the job's REC calls this.
template <int REC, class CodeAt, class VisAt>
__device__ __forceinline__ HmmStepSums hmm_decode_steps(const int slot, const int n, const HmmStepCarry cy, const unsigned long long gmask,
                                                        const uint32_t* l_rec, const uint32_t* l_info, const uint32_t* l_blocks, const int nb,
                                                        const uint8_t* motif_bytes, uint16_t* pbuf, const int pcap, CodeAt code_at, VisAt vis_at) {
  const int hwlane = (int)(threadIdx.x & 63u);
  const unsigned long long below = gmask & ((1ull << hwlane) - 1ull);
  const bool valid = slot < n;
  const int state = valid ? (int)l_rec[2 * slot] : 0, idx = valid ? (int)l_rec[2 * slot + 1] : 0;
  const uint32_t inf = valid ? l_info[state] : 0u;
  const int kind = (int)(inf & 7u), blk = (int)((inf >> 8) & 0xFFu), expected = (int)((inf >> 16) & 0xFFu);
  if (valid && pbuf && cy.np + slot < pcap) pbuf[pcap - 1 - (cy.np + slot)] = (uint16_t)state;
  // the state walked just before this one (the step before: the lane before)
  const int up = __shfl_up(state, 1);
  const int nxt = slot == 0 ? cy.nxt : up;
  // MotifStart (1) adds the implied leading deletions, Skip (3) / Mismatch / Ins (5) / Del (6) are edits, Skip / Match-state /
  // Del consume a reference base
  const int qbase = valid ? hmm_code_char(code_at(idx)) : 0;
  const int dels = kind == 1 ? nxt - state - 1 : 0;
  const int mism = kind == 4 && !(qbase == expected || expected == 'N');  // events.rs:66-73
  int edit = valid ? dels + (kind == 3) + mism + (kind == 5) + (kind == 6) : 0;
  int ref = valid ? dels + (kind == 3) + (kind == 4) + (kind == 6) : 0;
  // the last block end (2) walked before this step: the bases of the visit a block start (1) closes are query[idx .. vb1)
  const unsigned long long ends = __ballot(valid && kind == 2) & gmask, starts = __ballot(valid && kind == 1) & gmask;
  const unsigned long long ends_below = ends & below;
  const int src_end = ends_below ? 63 - (int)__builtin_clzll(ends_below) : hwlane;
  const int idx_end = __shfl(idx, src_end);
  const int vb1 = ends_below ? idx_end : cy.vb;
  if (valid && kind == 1) {  // a motif visit
    // remove_imperfect_motifs(.., 6) (operations.rs:45-57): only copies of STR motifs can be dropped -- short ones, and ones
    // whose bases differ from the motif (its bases are columns idx + 1 .. idx + mlen: in the window)
    uint32_t drop = 0;
    const int mlen = (int)l_blocks[2 * nb + blk];
    if (blk != nb - 1 && mlen <= 6) {
      if (vb1 - idx < mlen) drop = 1;
      else {
        const uint8_t* mot = motif_bytes + l_blocks[3 * nb + blk];
        for (int j = 0; j < mlen; ++j) {
          const int obs = hmm_code_char(code_at(idx + j + 1));
          if (mot[j] != 'N' && obs != mot[j]) drop = 1;
        }
      }
    }
    uint32_t* vrec = vis_at(cy.nv + (int)__builtin_popcountll(starts & below));
    vrec[0] = (uint32_t)blk | (drop << 15); vrec[1] = (uint32_t)idx; vrec[2] = (uint32_t)vb1;
  }
  // sums over the round (butterfly inside the job's lanes)
#pragma unroll
  for (int o = REC / 2; o >= 1; o >>= 1) { edit += __shfl_xor(edit, o); ref += __shfl_xor(ref, o); }
  const int src_last_end = ends ? 63 - (int)__builtin_clzll(ends) : hwlane;
  HmmStepSums r;
  r.edit = edit; r.ref = ref; r.n_starts = (int)__builtin_popcountll(starts);
  r.idx_last_end = __shfl(idx, src_last_end);
  r.last_state = __shfl(state, (hwlane & ~(REC - 1)) + max(n - 1, 0));
  r.any_end = ends != 0ull;
  return r;
}

// ---- state path: shift the reversed tail (np steps at the end of pbuf[pcap]) to the front (forward order)
template <class Sync>
__device__ __forceinline__ void hmm_path_to_front(const Sync sync, const int tid, const int nthr, uint16_t* pbuf, const int np, const int pcap) {
  if (!pbuf) return;
  const int n = min(np, pcap), shift = pcap - n;
  sync.mem();  // (the path was written by the decoding lanes)
  for (int base = 0; base < n; base += nthr) {
    const int f = base + tid;
    uint16_t v = 0;
    if (f < n) v = pbuf[shift + f];
    sync.mem();
    if (f < n) pbuf[f] = v;
    sync.mem();
  }
}

// ---- calc_purity (purity.rs:6-41) and the lengths that go with it; one thread
__device__ __forceinline__ void hmm_store_purity(const uint32_t job_index, const int np, const int edit, const int ref, const int qlen, uint32_t* path_len,
                                                 double* purity, int32_t* edit_out, int32_t* maxd_out) {
  if (path_len) path_len[job_index] = (uint32_t)np;
  const int mx = max(ref, qlen);
  purity[job_index] = ((double)mx - (double)edit) / (double)mx;
  if (edit_out) edit_out[job_index] = edit;
  if (maxd_out) maxd_out[job_index] = mx;
}

// ---- the trace-back word of state st (l.info): kind (0 outside any block, 1 block start, 2 block end, 3 skip state, 4 match, 5 insertion,
// 6 deletion) | emits << 3 | block << 8 | expected motif base << 16 (match states).  blk: the state's block (-1: none); blocks: [4][nb]
__device__ __forceinline__ uint32_t hmm_state_info(const int st, const int blk, const int nb, const uint32_t* blocks, const uint8_t* motif_bytes, const uint32_t flags_st) {
  uint32_t kind = 0, expected = 0;
  if (blk >= 0) {
    const int bstart = (int)blocks[0 * nb + blk], bend = (int)blocks[1 * nb + blk];
    if (st == bstart) kind = 1;
    else if (st == bend) kind = 2;
    else if (blk == nb - 1) kind = 3;
    else {
      const int mlen = (int)blocks[2 * nb + blk], off = st - bstart - 1, k = off / mlen;
      kind = 4u + (uint32_t)k;
      if (k == 0) expected = motif_bytes[blocks[3 * nb + blk] + off];
    }
  }
  return kind | ((flags_st & 1u) << 3) | ((uint32_t)(blk & 0xFF) << 8) | (expected << 16);
}

// ---- the serial trace-back of the fill kernels and of hmm_trace_ppl_kernel.  LDS of a job as they carve it up:
struct HmmTraceLds {
  int* tb;                  // the walk's state, shared between the walker (thread 0) and the stagers: the words TB_*
  const uint32_t* inst;     // [S][4] hmm_pred_entry
  const uint32_t* info;     // [S] the trace-back word of a state
  const uint32_t* blocks;   // [4][nb]
  const uint8_t* flags;     // [S]
  uint8_t* stage;           // staged back-pointer columns; afterwards the chunks of overflowed visits
  uint8_t* seq;             // symbol codes of the staged columns (+ HMM_CODE_PAD)
  const uint8_t* mot;       // motif bytes
  uint32_t* vis;            // [HMM_VIS_LDS][3] the first motif visits
  uint32_t* cnt;            // [n_motifs]
  uint32_t* rec;            // [REC][2] (state, column) of the steps of a round
};
enum { TB_STATE = 0, TB_IDX, TB_DONE, TB_NPATH, TB_NVISIT, TB_EDIT, TB_REF, TB_NEXT, TB_VB1,
       TB_NREC,   // steps noted in this round
       TB_MORE,   // 1: the chunk has more, 0: it is exhausted, 2: the walk is over
       TB_LOC };  // hmm_bp_loc of TB_STATE (packed rows)
__device__ __forceinline__ void hmm_trace_init(int* tb, const int S, const int L) {  // (thread 0) the walk starts in the end state, in the last column
  tb[TB_STATE] = S - 1; tb[TB_IDX] = L - 1; tb[TB_DONE] = 0; tb[TB_NPATH] = 0; tb[TB_NVISIT] = 0; tb[TB_EDIT] = 0; tb[TB_REF] = 0; tb[TB_NEXT] = -1; tb[TB_VB1] = 0;
}

// traceback (hmm_model.rs:125-142) fused with get_events/calc_purity (events.rs:17-86, purity.rs:6-41) and motif-visit collection
// (operations.rs:26-40); back-pointer columns are staged through LDS.
// Thread 0 only CHASES the back-pointers (state, column -> predecessor: two LDS round trips and a dozen instructions per step)
// and notes the states it passes, REC at a time; what each step means -- its events, its part of the edit count, the motif
// visit it closes -- is then worked out for all noted steps at once, one lane per step (hmm_decode_steps).  (Everything in one loop on
// one lane was 90 instructions per step: 750 cycles, a third of the kernel.)  What a step needs from its neighbours is little: the state
// walked just before it (the implied leading deletions of a block start) and the column of the last block end before it (the
// bases of the visit a block start closes): a lane shift and a ballot.
// PPL: the rows may be those of the position-per-lane fill, one byte per lane of the job's group (`packed`; TB_LOC is carried then);
// else they are one byte per state, `packed` is ignored, and the run end's back-pointer is guarded against a column no path goes through.
// VIS: motif visits the job keeps in LDS (l.vis); the others go to its workspace at their own index.
// CHUNK: 0, or (a job of REC lanes with packed rows of REC bytes) the most cols_per_chunk can be: a chunk is then staged with a fixed
// number of pieces per lane, every one loaded before the first is stored.
template <int REC, bool PPL, int VIS = HMM_VIS_LDS, int CHUNK = 0, class Sync>
__device__ __forceinline__ void hmm_trace_rounds(const Sync sync, const int tid, const int nthr, const HmmTraceLds l, const bool packed_arg, const int rstride,
                                                 const int cols_per_chunk, const int S, const int nb, const int L, const uint8_t* __restrict__ seq,
                                                 const uint8_t* bp, uint32_t* g_vis, uint16_t* pbuf, const int pcap, const unsigned long long gmask) {
  const bool packed = PPL && packed_arg;
  int* const tb = l.tb;
  while (true) {
    if (tb[TB_DONE]) break;
    const int c1 = tb[TB_IDX] + 1, c0 = packed ? (max(0, c1 - cols_per_chunk) & ~1) : max(0, c1 - cols_per_chunk);  // (rows of 8 bytes: an even column starts a 16-byte piece)
    if constexpr (CHUNK == 0) {
      const uint4* src = reinterpret_cast<const uint4*>(bp + (size_t)c0 * rstride);
      uint4* dst = reinterpret_cast<uint4*>(l.stage);
      const int n16 = ((c1 - c0) * rstride + 15) / 16;
      for (int i = tid; i < n16; i += nthr) dst[i] = src[i];
      // ... and the symbol codes of the same columns, plus those a motif copy starting in the last of them reaches into
      for (int k = tid; k < c1 - c0 + HMM_CODE_PAD && c0 + k < L; k += nthr) l.seq[k] = (uint8_t)hmm_code(seq, c0 + k, L);
    } else {
      // (the same copies with REC lanes: loops of one global round trip per pass were eleven passes for the codes of 64 columns and five
      //  for their rows; here the loads of a chunk are all in flight at once)
      constexpr int U16 = (((CHUNK + 1) * REC + 15) / 16 + REC - 1) / REC, UC = (CHUNK + 1 + HMM_CODE_PAD + REC - 1) / REC;
      const uint4* src = reinterpret_cast<const uint4*>(bp + (size_t)c0 * REC);
      uint4* dst = reinterpret_cast<uint4*>(l.stage);
      const int n16 = ((c1 - c0) * REC + 15) / 16, nc = min(c1 - c0 + HMM_CODE_PAD, L - c0);
      uint4 r16[U16];
      int rc[UC];
#pragma unroll
      for (int u = 0; u < U16; ++u) r16[u] = tid + u * REC < n16 ? src[tid + u * REC] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int u = 0; u < UC; ++u) rc[u] = tid + u * REC < nc ? hmm_code(seq, c0 + tid + u * REC, L) : 0;
#pragma unroll
      for (int u = 0; u < U16; ++u) if (tid + u * REC < n16) dst[tid + u * REC] = r16[u];
#pragma unroll
      for (int u = 0; u < UC; ++u) if (tid + u * REC < nc) l.seq[tid + u * REC] = (uint8_t)rc[u];
    }
    auto code_at = [&](int i) -> int { return (int)l.seq[i - c0]; };
    sync.lds();
    for (;;) {
      if (tid == 0) {  // ---- the chase
        int state = tb[TB_STATE], idx = tb[TB_IDX], n = 0;
        int row = (idx - c0) * rstride;  // offset of column idx in the staged chunk
        int emits = (int)((l.info[state] >> 3) & 1u);
        uint32_t loc = PPL ? (uint32_t)tb[TB_LOC] : 0u;
        while (state != 0 && idx >= c0 && n < REC) {
          l.rec[2 * n] = (uint32_t)state; l.rec[2 * n + 1] = (uint32_t)idx; ++n;
          const uint4 pred4 = *reinterpret_cast<const uint4*>(l.inst + 4 * state);  // all four predecessors: no second round trip behind b
          int b;
          if (packed) {
            b = (int)hmm_bp_unpack(l.stage[row + (int)(loc & 63u)], loc);
            if (state == S - 2) b = (int)hmm_bp_run_end(*reinterpret_cast<const uint32_t*>(l.stage + row));
          } else b = l.stage[row + state];
          uint32_t pe = (b & 2) ? ((b & 1) ? pred4.w : pred4.z) : ((b & 1) ? pred4.y : pred4.x);  // predecessor | its "emits" bit << 15 | its hmm_bp_loc << 16
          if (state == S - 2) {  // the run end: from a block end
            const int bb = PPL ? b : (b < nb ? b : 0);
            const uint32_t be_ = l.blocks[1 * nb + bb];
            pe = be_ | ((uint32_t)(l.flags[be_] & 1) << 15);
            if (PPL) pe |= hmm_bp_loc_block_end(bb, nb, l.blocks) << 16;
          }
          if (emits) { --idx; row -= rstride; }
          emits = (int)((pe >> 15) & 1u);
          state = (int)(pe & 0x7FFFu);
          loc = pe >> 16;
        }
        tb[TB_STATE] = state; tb[TB_IDX] = idx; tb[TB_NREC] = n;
        if (PPL) tb[TB_LOC] = (int)loc;
        tb[TB_MORE] = state == 0 ? 2 : (idx >= c0 ? 1 : 0);
      }
      sync.lds();
      const int more = tb[TB_MORE];  // (read before the next barrier: thread 0 writes it again right behind that one)
      if (tid < REC) {
        const int n = tb[TB_NREC];
        const HmmStepCarry cy{tb[TB_NPATH], tb[TB_NVISIT], tb[TB_NEXT], tb[TB_VB1]};
        // (the first VIS visits in LDS, the others in the job's workspace at their own index)
        const HmmStepSums r = hmm_decode_steps<REC>(tid, n, cy, gmask, l.rec, l.info, l.blocks, nb, l.mot, pbuf, pcap, code_at,
                                                    [&](int nv) -> uint32_t* { return nv < VIS ? l.vis + 3 * nv : g_vis + 3 * (size_t)nv; });
        if (tid == 0) {
          int np = cy.np + n;
          if (more == 2) { if (pbuf && np < pcap) pbuf[pcap - 1 - np] = 0; ++np; tb[TB_DONE] = 1; }
          tb[TB_NPATH] = np; tb[TB_NVISIT] = cy.nv + r.n_starts; tb[TB_EDIT] += r.edit; tb[TB_REF] += r.ref;
          if (n > 0) tb[TB_NEXT] = r.last_state;
          if (r.any_end) tb[TB_VB1] = r.idx_last_end;
        }
      }
      sync.lds();
      if (more != 1) break;
    }
  }
}

// ---- decode (thread 0): label_motifs over the kept copies, skip filter, counts, collapse.  Visits were recorded back to front: the
//      last ones recorded (the first of the allele) sit in global memory and come through LDS in chunks.  VIS: visits kept in LDS;
//      STAGE: bytes of the staging window l.stage, which takes the chunks.
template <int VIS = HMM_VIS_LDS, int STAGE = HMM_STAGE_BYTES, class Sync>
__device__ __forceinline__ void hmm_decode_visits(const Sync sync, const int tid, const int nthr, const HmmTraceLds l, const int nb, const uint32_t* g_vis,
                                                  int32_t* const sp, uint32_t* n_spans_job, uint32_t* counts_job) {
  const int n_motifs = nb - 1;
  int ns = 0, cum = 0, last_motif = -1, last_end = -1;
  auto take_visit = [&](const uint32_t* vrec) {
    const int blk = (int)(vrec[0] & 0x7FFFu), b0 = (int)vrec[1], b1 = (int)vrec[2];
    const bool keep = (vrec[0] >> 15) == 0;
    const int cnt = b1 - b0;
    const int start = cum, end = cum + cnt;
    cum = end;
    const int motif = keep ? blk : nb - 1;
    if (motif < n_motifs) {
      l.cnt[motif] += 1;
      if (ns > 0 && last_motif == motif && last_end == start) { sp[3 * (ns - 1) + 2] = end; }
      else { sp[3 * ns + 0] = motif; sp[3 * ns + 1] = start; sp[3 * ns + 2] = end; ++ns; last_motif = motif; }
      last_end = end;
    }
  };
  int v = l.tb[TB_NVISIT] - 1;
  constexpr int VIS_CHUNK = STAGE / 12;
  uint32_t* const l_vchunk = reinterpret_cast<uint32_t*>(l.stage);  // (the staging window of the back-pointers is free now)
  while (v >= VIS) {
    const int n = min(v - VIS + 1, VIS_CHUNK), v0 = v - n + 1;
    sync.mem();  // (the visits were written by the decoding lanes; the chunk before has been consumed)
    for (int k = tid; k < 3 * n; k += nthr) l_vchunk[k] = g_vis[3 * (size_t)v0 + k];
    sync.lds();
    if (tid == 0) for (int k = n - 1; k >= 0; --k) take_visit(l_vchunk + 3 * k);
    v -= n;
  }
  if (tid == 0) {
    for (; v >= 0; --v) take_visit(l.vis + 3 * v);
    *n_spans_job = (uint32_t)ns;
  }
  sync.lds();
  for (int m = tid; m < n_motifs; m += nthr) counts_job[m] = l.cnt[m];
}
