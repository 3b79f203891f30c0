// trgt_amd/csrc/wfa_win.hip -- wfa_win_kernel: the windowed flank alignments of trgt_find_spans_batch (spans.hip: piece_window,
// flank_window_kernel) on ONE wave each, wavefronts and their whole history in registers.
//
// A window job is a flank piece against a few hundred read bases, started on the diagonals [0, text_begin_free] only and given up
// above the penalty S0 <= 15 the window argument covers.  Its wavefronts never leave the diagonals [-S0, text_begin_free + S0]: with
// two diagonals per lane (diagonal WIN_KBASE + 2 lane in the low half of a dword, the next one in the high half) the M, I and D
// offsets of ALL levels 0..S0 are 16 + 15 + 15 registers per lane, and that array is the recurrence's ring and the back-trace's
// history at once.  Same arithmetic as wf_run_lds_affine<64, true> / wf_backtrace_fast_affine (wfa_fast.hpp) in the same encoding
// (offset + 1, 0 = NULL), so the same co-optimal alignment is chosen:
//   * recurrence on packed 16-bit pairs, neighbour diagonals by DPP wave shifts;
//   * wavefront_compute_trim_ends: a source outside the trimmed range of its wavefront reads as NULL.  M cells out of bounds are
//     stored as NULL anyway; I and D cells outside [first, last in-bounds cell] of their level are cleared when the level is stored,
//     which is the same thing for every later reader (recurrence and back-trace alike);
//   * a cell outside the range wavefront_compute_limits_input would give the level has no source and computes to NULL by itself;
//   * termination: the lowest diagonal whose cell has consumed the pattern (pattern ends fixed, text ends free);
//   * back-trace: (offset << 4 | type), the maximum wins.  Every step lowers the level, so the walk is unrolled over the levels from
//     S0 down and every history register is named at compile time (no scratch); the cell of a diagonal comes by v_readlane.  All
//     of its state is wave-uniform.  Only what the locus path reads is kept: matches, the pattern / text span of the M and X
//     operations, the penalty.
// Piece and window are staged once in LDS as plain bytes (one 8-byte global load per lane and sequence, 1 KB per wave); a 4-base
// window of the extension is two aligned dwords (one ds_read2_b32) and a v_alignbyte.  Straight from global memory the same window
// would be one unaligned dword, but every extension step is a dependent round trip -- ~16 levels x 1-3 steps per job -- and the
// vector L1's latency is several times the LDS's; the LDS copy costs two loads and two stores per lane and job.
// No workspace slot, no history arena, no descriptors, no barrier.  A job the layout cannot hold (sequences beyond the staging
// buffers) gets the "not completed" score, is counted (SpanCount::SC_WINFALL) and is aligned against the whole read by the rest
// launch like every window that does not stand (window_check_kernel).
#include "wfa_host.hpp"

namespace trgt {
namespace {

constexpr int WIN_LEVELS = 16;     // levels 0 .. 15 in registers
constexpr int WIN_KBASE = -16;     // diagonal of lane 0's low half
constexpr int WIN_SEQ_CAP = 496;   // longest piece / window the staging buffers take
constexpr int WIN_SEQ_DW = 132;    // dwords per staged sequence: 512 bytes written by the 64 lanes + slack for the window behind the end
constexpr int WIN_CLAIM = 4;       // jobs per atomic (wfa_fast.hpp: the rate of same-address atomics bounds a launch of 3-us jobs)

struct WinKArgs {
  const JobDev* jobs; const uint32_t* n_jobs_dev;
  const uint8_t* pat_base; const uint8_t* txt_base;
  unsigned int* counter;       // job claims
  unsigned int* fallback;      // jobs not taken
  int32_t* score; int32_t* n_match; uint32_t* span4;  // by JobDev::out_index
  int32_t tbf, s_max;          // text_begin_free; last level (<= WIN_LEVELS - 1)
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t wpk_max(uint32_t a, uint32_t b) { union { uint32_t u; us2 v; } x, y, r; x.u = a; y.u = b; r.v = __builtin_elementwise_max(x.v, y.v); return r.u; }
__device__ __forceinline__ uint32_t wpk_min(uint32_t a, uint32_t b) { union { uint32_t u; us2 v; } x, y, r; x.u = a; y.u = b; r.v = __builtin_elementwise_min(x.v, y.v); return r.u; }
__device__ __forceinline__ uint32_t wpk_add(uint32_t a, uint32_t b) { union { uint32_t u; us2 v; } x, y, r; x.u = a; y.u = b; r.v = x.v + y.v; return r.u; }
__device__ __forceinline__ uint32_t wpk_inc_nz(uint32_t x) { return wpk_add(x, wpk_min(x, 0x00010001u)); }  // + 1 unless NULL, both halves
__device__ __forceinline__ uint32_t win_ffbl(uint32_t v) {  // v_ffbl_b32: -1 for 0 ("no mismatch in this window")
  uint32_t r;
  asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v));
  return r;
}
// lane i <- x[i - 1], lane 0 <- 0 / lane i <- x[i + 1], lane 63 <- 0
__device__ __forceinline__ uint32_t lane_below(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }
__device__ __forceinline__ uint32_t lane_above(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130 /* wave_shl:1 */, 0xF, 0xF, false); }
__device__ __forceinline__ int win_rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

// bytes i .. i + 3 of a staged sequence
__device__ __forceinline__ uint32_t seq_window(const uint32_t* S, int i) {
  const int d = i >> 2;
  return __builtin_amdgcn_alignbyte(S[d + 1], S[d], (uint32_t)i & 3u);
}
// The 64 lanes copy a sequence of 8 .. WIN_SEQ_CAP bytes to LDS, eight bytes each, zeros behind its end; nothing is read beyond the sequence.
__device__ __forceinline__ void stage_bytes(const uint8_t* __restrict__ src, int len, uint32_t* S, int lane) {
  const int i0 = 8 * lane;
  uint64_t w = 0;
  if (i0 + 8 <= len) __builtin_memcpy(&w, src + i0, 8);
  else if (i0 < len) { __builtin_memcpy(&w, src + len - 8, 8); w >>= 8 * (8 - (len - i0)); }  // the eight bytes that END the sequence
  S[2 * lane] = (uint32_t)w; S[2 * lane + 1] = (uint32_t)(w >> 32);
  if (lane < WIN_SEQ_DW - 128) S[128 + lane] = 0u;
}

// candidate of the back-trace: the cell of diagonal k in a history register, (offset + add) << 4 | type, -1 when NULL
__device__ __forceinline__ int bt_cand(uint32_t reg, int k, int add, int type) {
  const int idx = k - WIN_KBASE;
  if (idx < 0 || idx > 127) return -1;
  const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)reg, idx >> 1);
  const uint32_t enc = (idx & 1) ? r >> 16 : r & 0xFFFFu;
  return enc == 0u ? -1 : (int)(((enc - 1u + (uint32_t)add) << 4) | (uint32_t)type);
}

__global__ void __launch_bounds__(64) wfa_win_kernel(const WinKArgs a) {
  __shared__ uint32_t lds_seq[2 * WIN_SEQ_DW];
  uint32_t* const Pq = lds_seq;
  uint32_t* const Tq = lds_seq + WIN_SEQ_DW;
  const int lane = threadIdx.x;
  const int kA = WIN_KBASE + 2 * lane, kB = kA + 1;
  const uint32_t n_jobs = *a.n_jobs_dev;
  const int s_max = a.s_max;
  uint32_t next = 0, chunk_end = 0;
  for (;;) {
    if (next >= chunk_end) {
      uint32_t b = 0;
      if (lane == 0) b = atomicAdd(a.counter, (unsigned)WIN_CLAIM);
      next = (uint32_t)win_rfl((int)b); chunk_end = next + WIN_CLAIM;
    }
    const uint32_t j = next++;
    if (j >= n_jobs) break;
    const JobDev job = a.jobs[j];
    const int plen = win_rfl((int)job.pat_len), tlen = win_rfl((int)job.txt_len);
    const uint32_t o = (uint32_t)win_rfl((int)job.out_index);
    if (plen < 8 || tlen < 8 || plen > WIN_SEQ_CAP || tlen > WIN_SEQ_CAP) {  // not taken: the rest launch aligns it against the whole read
      if (lane == 0) { a.score[o] = INT32_MIN; a.n_match[o] = 0; atomicAdd(a.fallback, 1u); }
      continue;
    }
    stage_bytes(a.pat_base + job.pat_off, plen, Pq, lane);
    stage_bytes(a.txt_base + job.txt_off, tlen, Tq, lane);
    asm volatile("" ::: "memory");  // (one wave: LDS operations complete in order, nothing to wait for)
    const int tbf = min(a.tbf, tlen);

    // one extension step of a cell at (v, h): the matching bases of the next four
    auto step4 = [&](int v, int h) -> uint32_t {
      const uint32_t xw = seq_window(Pq, v) ^ seq_window(Tq, h);
      return min(min(win_ffbl(xw) >> 3, 4u), (uint32_t)min(plen - v, tlen - h));
    };
    // the rest of a long run of matches, by the whole wave: lane i compares the window 4 i bases further on (wfa_fast.hpp: finish_runs)
    auto finish_runs = [&](bool c, int& v, int& h) {
      unsigned long long m = __ballot(c);
      while (m) {
        const int jl = (int)__builtin_ctzll(m);
        m &= m - 1ull;
        int vj = __builtin_amdgcn_readlane(v, jl), hj = __builtin_amdgcn_readlane(h, jl);
        for (;;) {
          const int pv = vj + 4 * lane, ph = hj + 4 * lane;
          const int rem = min(plen - pv, tlen - ph);
          const uint32_t xw = seq_window(Pq, min(pv, plen)) ^ seq_window(Tq, min(ph, tlen));
          const uint32_t n = rem > 0 ? min(min(win_ffbl(xw) >> 3, 4u), (uint32_t)rem) : 0u;
          const unsigned long long stop = __ballot(n < 4u);
          if (stop) {
            const int js = (int)__builtin_ctzll(stop);
            const int ext = 4 * js + __builtin_amdgcn_readlane((int)n, js);
            vj += ext; hj += ext;
            break;
          }
          vj += 256; hj += 256;
        }
        if (lane == jl) { v = vj; h = hj; }
      }
    };
    // extend the two cells of a lane (okA / okB: the cell exists) from offsets offA / offB; returns the packed M entry
    auto extend2 = [&](bool okA, bool okB, int offA, int offB, bool& termA, bool& termB) -> uint32_t {
      int vA = okA ? offA - kA : 0, hA = okA ? offA : 0, vB = okB ? offB - kB : 0, hB = okB ? offB : 0;
      uint32_t nA = step4(vA, hA), nB = step4(vB, hB);
      vA += (int)nA; hA += (int)nA; vB += (int)nB; hB += (int)nB;
      bool cA = okA && nA == 4u, cB = okB && nB == 4u;
      if (__ballot(cA || cB)) {
        if (cA) { nA = step4(vA, hA); vA += (int)nA; hA += (int)nA; cA = nA == 4u; }
        if (cB) { nB = step4(vB, hB); vB += (int)nB; hB += (int)nB; cB = nB == 4u; }
        finish_runs(cA, vA, hA);
        finish_runs(cB, vB, hB);
      }
      termA = okA && vA >= plen; termB = okB && vB >= plen;  // wavefront_termination_endsfree: pattern ends fixed, text end free
      return (okA ? (uint32_t)hA + 1u : 0u) | ((okB ? (uint32_t)hB + 1u : 0u) << 16);
    };
    // I / D entries of a level: cleared outside [first, last] in-bounds cell (wavefront_compute_trim_ends)
    auto trimmed = [&](uint32_t pk) -> uint32_t {
      const uint32_t eA = (pk & 0xFFFFu) - 1u, eB = (pk >> 16) - 1u;
      const bool inA = eA <= (uint32_t)tlen && (eA - (uint32_t)kA) <= (uint32_t)plen, inB = eB <= (uint32_t)tlen && (eB - (uint32_t)kB) <= (uint32_t)plen;
      const unsigned long long bA = __ballot(inA), bB = __ballot(inB);
      if ((bA | bB) == 0ull) return 0u;
      const int fA = bA ? 2 * (int)__builtin_ctzll(bA) : 256, fB = bB ? 2 * (int)__builtin_ctzll(bB) + 1 : 256;
      const int lA = bA ? 2 * (63 - (int)__builtin_clzll(bA)) : -1, lB = bB ? 2 * (63 - (int)__builtin_clzll(bB)) + 1 : -1;
      const int first = min(fA, fB), last = max(lA, lB);
      const bool keepA = 2 * lane >= first && 2 * lane <= last, keepB = 2 * lane + 1 >= first && 2 * lane + 1 <= last;
      return (keepA ? pk & 0xFFFFu : 0u) | (keepB ? pk & 0xFFFF0000u : 0u);
    };

    uint32_t M[WIN_LEVELS], I[WIN_LEVELS], D[WIN_LEVELS];
#pragma unroll
    for (int s = 0; s < WIN_LEVELS; ++s) { M[s] = 0u; I[s] = 0u; D[s] = 0u; }
    int end_s = -1, end_k = 0, end_off = 0;
    auto terminated = [&](int s, uint32_t mq, bool termA, bool termB) -> bool {  // the lowest terminating diagonal ends the alignment
      const unsigned long long tA = __ballot(termA), tB = __ballot(termB);
      if ((tA | tB) == 0ull) return false;
      const int la = tA ? (int)__builtin_ctzll(tA) : 64, lb = tB ? (int)__builtin_ctzll(tB) : 64;
      const bool isA = la <= lb;
      const int l = isA ? la : lb;
      const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)mq, l);
      end_s = s; end_k = WIN_KBASE + 2 * l + (isA ? 0 : 1); end_off = (int)(isA ? r & 0xFFFFu : r >> 16) - 1;
      return true;
    };
    // ---- level 0: the diagonals [0, text_begin_free], never trimmed
    {
      bool tA, tB;
      M[0] = extend2(kA >= 0 && kA <= tbf, kB >= 0 && kB <= tbf, kA, kB, tA, tB);
      terminated(0, M[0], tA, tB);
    }
    // ---- levels 1 .. s_max (x, o + e, e = 2, 6, 1)
#pragma unroll
    for (int s = 1; s < WIN_LEVELS; ++s) {
      if (end_s >= 0 || s > s_max) break;
      const uint32_t Mm = s >= 2 ? M[s - 2] : 0u, Mo = s >= 6 ? M[s - 6] : 0u, Ie = I[s - 1], De = D[s - 1];
      const uint32_t insS = wpk_max(__builtin_amdgcn_alignbit(Mo, lane_below(Mo), 16), __builtin_amdgcn_alignbit(Ie, lane_below(Ie), 16));  // sources at k - 1
      const uint32_t del = wpk_max(__builtin_amdgcn_alignbit(lane_above(Mo), Mo, 16), __builtin_amdgcn_alignbit(lane_above(De), De, 16));   // sources at k + 1
      const uint32_t ins = wpk_inc_nz(insS), mis = wpk_inc_nz(Mm);
      const uint32_t mxp = wpk_max(del, wpk_max(mis, ins));
      const int offA = (int)(mxp & 0xFFFFu) - 1, offB = (int)(mxp >> 16) - 1;
      const bool okA = (uint32_t)offA <= (uint32_t)tlen && (uint32_t)(offA - kA) <= (uint32_t)plen;
      const bool okB = (uint32_t)offB <= (uint32_t)tlen && (uint32_t)(offB - kB) <= (uint32_t)plen;
      if (__ballot(mxp != 0u) == 0ull) continue;  // a level without sources: all NULL
      bool tA, tB;
      M[s] = extend2(okA, okB, offA, offB, tA, tB);
      I[s] = trimmed(ins); D[s] = trimmed(del);
      terminated(s, M[s], tA, tB);
    }
    if (end_s < 0) {  // penalty above s_max: the window does not stand
      if (lane == 0) { a.score[o] = INT32_MIN; a.n_match[o] = 0; }
      continue;
    }
    // ---- back-trace (wf_backtrace_fast_affine), wave-uniform
    int s = end_s, k = end_k, off = end_off;
    int h = off, v = off - k;
    int nm = 0, ps = 0, pe = 0, ts = 0, te = 0;
    bool gap = false, del_gap = false, started = false, live = true;
    auto match_run = [&](int len) {  // M / X operations ending at (v, h)
      if (!started) { pe = v; te = h; started = true; }
      ps = v - len; ts = h - len;
    };
#pragma unroll
    for (int L = WIN_LEVELS - 1; L >= 1; --L) {
      if (!(live && s == L && v > 0 && h > 0)) continue;
      if (!gap) {
        int best = L >= 2 ? bt_cand(M[L - 2], k, 1, 9) : -1;
        best = max(best, bt_cand(D[L - 1], k + 1, 0, 6));
        if (L >= 6) best = max(best, bt_cand(M[L - 6], k + 1, 0, 5));
        best = max(best, bt_cand(I[L - 1], k - 1, 1, 2));
        if (L >= 6) best = max(best, bt_cand(M[L - 6], k - 1, 1, 1));
        if (best < 0) { live = false; continue; }
        const int best_off = best >> 4, type = best & 0xF;
        if (off > best_off) { match_run(off - best_off); nm += off - best_off; }
        off = best_off; h = off; v = off - k;
        if (v <= 0 || h <= 0) { live = false; continue; }
        switch (type) {
          case 9: match_run(1); s -= 2; --off; break;
          case 1: s -= 6; --k; --off; break;
          case 2: s -= 1; gap = true; del_gap = false; --k; --off; break;
          case 5: s -= 6; ++k; break;
          default: s -= 1; gap = true; del_gap = true; ++k; break;
        }
      } else {
        const int ce = del_gap ? bt_cand(D[L - 1], k + 1, 0, 6) : bt_cand(I[L - 1], k - 1, 1, 2);
        const int co = L >= 6 ? (del_gap ? bt_cand(M[L - 6], k + 1, 0, 5) : bt_cand(M[L - 6], k - 1, 1, 1)) : -1;
        if (max(ce, co) < 0) { live = false; continue; }
        if (ce > co) s -= 1; else { s -= 6; gap = false; }
        if (del_gap) ++k; else { --k; --off; }
      }
      h = off; v = off - k;
    }
    if (!gap && v > 0 && h > 0) { const int n = min(v, h); match_run(n); nm += n; }
    if (lane == 0) {
      a.score[o] = -end_s; a.n_match[o] = nm;
      *reinterpret_cast<uint4*>(a.span4 + 4 * (size_t)o) = make_uint4((uint32_t)ps, (uint32_t)pe, (uint32_t)ts, (uint32_t)te);
    }
  }
}

}  // namespace

bool wfa_win_fits(int mism, int gapo, int gape, int tbf, int s_max, int64_t max_plen, int64_t max_tlen) {
  // level s lives on the diagonals [-s, text_begin_free + s]; the lanes hold [WIN_KBASE, WIN_KBASE + 127]
  return preset_wgs(mism, gapo, gape) && s_max >= 1 && s_max <= WIN_LEVELS - 1 && s_max <= -WIN_KBASE && tbf >= 0 &&
         tbf + s_max <= WIN_KBASE + 127 && max_plen >= 8 && max_plen <= WIN_SEQ_CAP && max_tlen <= WIN_SEQ_CAP;
}

int wfa_win_launch(trgt_hip_ctx* c, const WfaWinLaunch& L) {
  if (!wfa_win_fits(2, 5, 1, L.tbf, L.s_max, 8, 8))
    return fail(c, TRGT_ERR_INVALID, "wfa_win: penalty bound %d / text_begin_free %d outside the register layout", L.s_max, L.tbf);
  WinKArgs a;
  a.jobs = L.jobs_dev; a.n_jobs_dev = L.n_jobs_dev; a.pat_base = L.pat_base; a.txt_base = L.txt_base;
  a.counter = L.counter; a.fallback = L.fallback; a.score = L.score; a.n_match = L.n_match; a.span4 = L.span4;
  a.tbf = L.tbf; a.s_max = L.s_max;
  // persistent one-wave workgroups, as many as can be resident; the number of jobs is known on the device only
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, wfa_win_kernel, 64, 0) != hipSuccess || occ < 1) { (void)hipGetLastError(); occ = 8; }
  occ = std::min(occ, 16);
  const int64_t per_claim = (L.n_jobs_host + WIN_CLAIM - 1) / WIN_CLAIM;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)c->num_cus * occ, per_claim));
  if (c->knobs.debug) fprintf(stderr, "[wfa] windowed launch in registers: occupancy=%d grid=%lld\n", occ, (long long)grid);
  KTimer t(c, L.timer_slot);
  hipLaunchKernelGGL(wfa_win_kernel, dim3((unsigned)grid), dim3(64), 0, c->stream, a);
  TRGT_HIP_TRY(c, hipGetLastError());
  t.stop(0);
  return TRGT_OK;
}

}  // namespace trgt
