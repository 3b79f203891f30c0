// trgt_amd/csrc/wfa_band.hip -- wfa_band_kernel: the banded alignments of what the pre-filter keeps (spans.hip: BandArgs) on ONE wave
// each, forward only: no history, no back-trace.
//
// A band job is a flank piece of at most BAND_PLEN_MAX bases against the text window [k_end - s*, k_end + s* + plen) of its read, started
// on the diagonals [0, tbf] (tbf <= 2 s*) and run up to the penalty s* <= BAND_CAP the pre-filter found.  Its wavefronts stay on the
// diagonals [-s*, tbf + s*]: every lane holds NPL consecutive diagonals (-s* + NPL lane + d; NPL = 2, 4, 6 or BAND_NPL, the fewest that
// hold the job's band), so neighbour diagonals are in-lane except at the two ends of the block, which one DPP wave shift per component
// and level serves.
//
// Same arithmetic as wf_run_lds_affine<64, true> (wfa_fast.hpp) in the same encoding (offset + 1, 0 = NULL), penalties (2, 5, 1):
//   * ins = max(M[s-6][k-1], I[s-1][k-1]) + 1, del = max(M[s-6][k+1], D[s-1][k+1]), mis = M[s-2][k] + 1, M = extend(max of the three);
//   * M cells out of bounds are stored as NULL; I and D cells outside [first, last] in-bounds cell of their level are cleared when the
//     level is stored (wavefront_compute_trim_ends); a cell without a source computes to NULL by itself (limits of the input);
//   * termination: the lowest diagonal whose cell has consumed the pattern (pattern ends fixed, text ends free).
// wf_backtrace_fast_affine walks back from the end cell by one choice per cell: the maximum of (offset << 4 | type) over the candidate
// sources -- mismatch 9 > deletion extended 6 > opened 5 > insertion extended 2 > opened 1.  Those candidates are the very values the
// recurrence holds when it computes the cell, so the choice is made HERE, going forward: every cell carries a summary of the path the
// back-trace would walk from it, taken from the source that wins under that rule (ties: I / D extension before M, then mis > del > ins)
// and updated by the operation and by the extension.  The summary is what the locus path reads of an alignment (the epilogue loop of
// wfa_fast_kernel): the matches, and the pattern position / diagonal at the start of the first and behind the last M or X operation.
// The back-trace stops at a cell with v <= 0 or h <= 0 (what is left is a leading gap): a source there hands on an empty summary.
// A cell is two dwords:
//   a: offset + 1 (bits 0-15) | matches (16-23) | pattern position of the first M / X (24-31)
//   b: pattern position behind the last M / X (0-7) | its diagonal (17-25) | diagonal of the first (8-16) | any M / X yet (26)
// (diagonals biased by s*, lane 0's first).  The ring is M of the levels s-1 .. s-6 and I, D of s-1, all in registers, ordered by age and moved
// down by one level per turn.  Piece and window are staged as plain bytes in LDS (wfa_win.hip).
// No workspace slot, no arena, no descriptors, no barrier.
//
// Per job the kernel does what heavy_band_kernel did in front of the LDS launch (s*, k_end from JobDev::pad, window and free text start)
// and what band_check_kernel did behind it (the penalty must come out as s* with n_match > 0, the window start is added to the text
// span; anything else goes to the whole-read list and is counted).  A banded job the layout cannot hold (s* > BAND_CAP, a piece beyond
// BAND_PLEN_MAX) goes to the fallback list for the LDS launch.
#include "wfa_host.hpp"

namespace trgt {
namespace {

constexpr int BAND_NPL = 7;                  // most diagonals per lane
constexpr int BAND_CAP = WFA_BAND_S_CAP;     // highest penalty: 4 BAND_CAP + 1 <= 64 BAND_NPL diagonals
constexpr int BAND_PLEN_MAX = WFA_BAND_PLEN_MAX;
constexpr int BAND_SEQ_DW = 132;             // dwords per staged sequence: 512 bytes written by the 64 lanes + slack for the window behind the end
static_assert(4 * BAND_CAP + 1 <= 64 * BAND_NPL, "the band of the highest penalty must fit the lanes");
static_assert(BAND_PLEN_MAX + 2 * BAND_CAP <= 504, "the window of the highest penalty must fit the staging buffer");
static_assert(64 * BAND_NPL <= 512 && BAND_PLEN_MAX <= 255, "summary fields: 9-bit diagonals, 8-bit pattern positions");

struct BandKArgs {
  const JobDev* jobs; const uint32_t* n_jobs_dev;  // the kept list
  const uint8_t* pat_base; const uint8_t* txt_base;
  uint32_t* count; int32_t i_claim, i_reg, i_fall, i_rest, i_fail;  // words of the call's counter block
  JobDev* fall_jobs; JobDev* rest_jobs;
  int32_t* n_match; uint32_t* span4;  // by JobDev::out_index
  const uint64_t* read_off; const uint32_t* read_len;
  int32_t s_max;  // the plan's bound on a banded penalty (jobs above it: whole read)
};

constexpr uint32_t B_PE = 0xFFu, B_KL = 0x1FFu << 17, B_STARTED = 1u << 26;

__device__ __forceinline__ uint32_t band_ffbl(uint32_t v) {  // v_ffbl_b32: -1 for 0 ("no mismatch in this window")
  uint32_t r;
  asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v));
  return r;
}
// lane i <- x[i - 1], lane 0 <- 0 / lane i <- x[i + 1], lane 63 <- 0
__device__ __forceinline__ uint32_t band_below(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }
__device__ __forceinline__ uint32_t band_above(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130 /* wave_shl:1 */, 0xF, 0xF, false); }
__device__ __forceinline__ int band_rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t band_enc(uint32_t a) { return a & 0xFFFFu; }

// bytes i .. i + 3 of a staged sequence
__device__ __forceinline__ uint32_t band_window(const uint32_t* S, int i) {
  const int d = i >> 2;
  return __builtin_amdgcn_alignbyte(S[d + 1], S[d], (uint32_t)i & 3u);
}
// The 64 lanes copy a sequence of 1 .. 504 bytes to LDS, eight bytes each, zeros behind its end; nothing is read beyond the sequence.
__device__ __forceinline__ void band_stage(const uint8_t* __restrict__ src, int len, uint32_t* S, int lane) {
  const int i0 = 8 * lane;
  uint64_t w = 0;
  if (i0 + 8 <= len) __builtin_memcpy(&w, src + i0, 8);
  else if (i0 < len) {
    if (len >= 8) { __builtin_memcpy(&w, src + len - 8, 8); w >>= 8 * (8 - (len - i0)); }  // the eight bytes that END the sequence
    else for (int b = 0; b < len; ++b) w |= (uint64_t)src[b] << (8 * b);                   // (lane 0 alone)
  }
  S[2 * lane] = (uint32_t)w; S[2 * lane + 1] = (uint32_t)(w >> 32);
  if (lane < BAND_SEQ_DW - 128) S[128 + lane] = 0u;
}

// One job on NPL diagonals per lane, kbase + NPL lane + d: the band [-s*, tbf + s*] needs tbf + 2 s* + 1 of them, and the cost of a level is
// the cost of NPL diagonals whatever lives on them, so a job takes the smallest instantiation that holds its band.  Leaves the level the
// alignment ended on (-1: not up to s*) and the end cell.
struct BandEnd { int s; uint32_t a, b; };  // wave-uniform
template <int NPL>
__device__ __forceinline__ BandEnd band_run(const uint32_t* Pq, const uint32_t* Tq, const int lane, const int plen, const int tlen, const int tbf, const int s_star,
                                            const int kbase) {
  int end_s = -1; uint32_t end_a = 0, end_b = 0;
  int ln = lane;
  asm volatile("" : "+v"(ln));  // (else the per-lane constants of all instantiations are hoisted out of the job loop together: 38 registers, and a spill)
  const int kA = kbase + NPL * ln, kbA = NPL * ln;  // first diagonal of the lane, plain and biased by -kbase
  // one extension step of a cell at (v, h): the matching bases of the next four
  auto step4 = [&](int v, int h) -> uint32_t {
    const uint32_t xw = band_window(Pq, v) ^ band_window(Tq, h);
    return min(min(band_ffbl(xw) >> 3, 4u), (uint32_t)min(plen - v, tlen - h));
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
        const uint32_t xw = band_window(Pq, min(pv, plen)) ^ band_window(Tq, min(ph, tlen));
        const uint32_t n = rem > 0 ? min(min(band_ffbl(xw) >> 3, 4u), (uint32_t)rem) : 0u;
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
  // The M cells of a level from their values before the extension (pa, pb: cell and summary of the winning source, operation applied):
  // bounds, extension, the extension's matches into the summary.  Leaves the cells in (pa, pb); returns whether any cell of the lane
  // has consumed the pattern (term[d]).
  auto extend_cells = [&](uint32_t (&pa)[NPL], uint32_t (&pb)[NPL], bool (&term)[NPL]) -> bool {
    int v[NPL], h[NPL], h0[NPL];
    bool ok[NPL], c[NPL];
    bool any = false;
#pragma unroll
    for (int d = 0; d < NPL; ++d) {
      const int k = kA + d, hp = (int)band_enc(pa[d]) - 1, vp = hp - k;
      ok[d] = (uint32_t)hp <= (uint32_t)tlen && (uint32_t)vp <= (uint32_t)plen;
      v[d] = ok[d] ? vp : 0; h[d] = ok[d] ? hp : 0; h0[d] = h[d];
      const uint32_t n = step4(v[d], h[d]);
      v[d] += (int)n; h[d] += (int)n;
      c[d] = ok[d] && n == 4u;
      any = any || c[d];
    }
    if (__ballot(any)) {
#pragma unroll
      for (int d = 0; d < NPL; ++d) {
        if (c[d]) { const uint32_t n = step4(v[d], h[d]); v[d] += (int)n; h[d] += (int)n; c[d] = n == 4u; }
        finish_runs(c[d], v[d], h[d]);
      }
    }
    bool t = false;
#pragma unroll
    for (int d = 0; d < NPL; ++d) {
      const uint32_t kb = (uint32_t)(kbA + d), ext = (uint32_t)(h[d] - h0[d]);
      uint32_t qa = (pa[d] & 0xFFFF0000u) + (ext << 16) + (uint32_t)h[d] + 1u, qb = pb[d];
      if (ext) {  // matches: an M run from (v - ext, h - ext) to (v, h)
        if (!(qb & B_STARTED)) { qa = (qa & 0x00FFFFFFu) | ((uint32_t)(v[d] - (int)ext) << 24); qb = (kb << 8) | B_STARTED; }
        qb = (qb & ~(B_PE | B_KL)) | (uint32_t)v[d] | (kb << 17);
      }
      pa[d] = ok[d] ? qa : 0u; pb[d] = ok[d] ? qb : 0u;
      term[d] = ok[d] && v[d] >= plen;  // wavefront_termination_endsfree: pattern ends fixed, text end free
      t = t || term[d];
    }
    return t;
  };
  // I / D cells of a level: cleared outside [first, last] in-bounds cell (wavefront_compute_trim_ends)
  auto trim = [&](uint32_t (&xa)[NPL], uint32_t (&xb)[NPL]) {
    int fd = NPL, ld = -1;
#pragma unroll
    for (int d = NPL - 1; d >= 0; --d) {
      const uint32_t e = band_enc(xa[d]) - 1u;
      const bool in = e <= (uint32_t)tlen && (e - (uint32_t)(kA + d)) <= (uint32_t)plen;
      fd = in ? d : fd; ld = in && ld < 0 ? d : ld;
    }
    const unsigned long long bl = __ballot(fd < NPL);
    int first = 64 * NPL, last = -1;
    if (bl) {
      const int fl = (int)__builtin_ctzll(bl), ll = 63 - (int)__builtin_clzll(bl);
      first = NPL * fl + __builtin_amdgcn_readlane(fd, fl); last = NPL * ll + __builtin_amdgcn_readlane(ld, ll);
    }
#pragma unroll
    for (int d = 0; d < NPL; ++d) {
      const bool keep = kbA + d >= first && kbA + d <= last;
      xa[d] = keep ? xa[d] : 0u; xb[d] = keep ? xb[d] : 0u;
    }
  };
  // the lowest terminating diagonal ends the alignment
  auto terminated = [&](int s, bool t, const uint32_t (&pa)[NPL], const uint32_t (&pb)[NPL], const bool (&term)[NPL]) {
    const unsigned long long tb = __ballot(t);
    if (!tb) return;
    uint32_t ta = 0, tq = 0;
#pragma unroll
    for (int d = NPL - 1; d >= 0; --d) { ta = term[d] ? pa[d] : ta; tq = term[d] ? pb[d] : tq; }
    const int l = (int)__builtin_ctzll(tb);
    end_a = (uint32_t)__builtin_amdgcn_readlane((int)ta, l); end_b = (uint32_t)__builtin_amdgcn_readlane((int)tq, l);
    end_s = s;
  };

  // ring by age: Ma / Mb[a] is M of level s - 1 - a (NULL below level 0), I and D of level s - 1; level s moves in at the end of its turn
  uint32_t Ma[6][NPL], Mb[6][NPL], Ia[NPL], Ib[NPL], Da[NPL], Db[NPL];
#pragma unroll
  for (int d = 0; d < NPL; ++d) {
#pragma unroll
    for (int r = 0; r < 6; ++r) { Ma[r][d] = 0u; Mb[r][d] = 0u; }
    Ia[d] = 0u; Ib[d] = 0u; Da[d] = 0u; Db[d] = 0u;
  }
  // ---- levels 0 .. s* (x, o + e, e = 2, 6, 1).  One body for all levels (not unrolled over the ring: six copies of it are the whole
  //      instruction cache): level 0 has no sources and takes the diagonals [0, text_begin_free] instead, never trimmed
#pragma nounroll
  for (int s = 0; s <= s_star && end_s < 0; ++s) {
    // the better of I[s-1][k] / M[s-6][k] and of D[s-1][k] / M[s-6][k], per diagonal (ties: the gap extension)
    uint32_t gIa[NPL], gIb[NPL], gDa[NPL], gDb[NPL];
#pragma unroll
    for (int d = 0; d < NPL; ++d) {
      const uint32_t mo = band_enc(Ma[5][d]);
      const bool ti = band_enc(Ia[d]) >= mo, td = band_enc(Da[d]) >= mo;
      gIa[d] = ti ? Ia[d] : Ma[5][d]; gIb[d] = ti ? Ib[d] : Mb[5][d];
      gDa[d] = td ? Da[d] : Ma[5][d]; gDb[d] = td ? Db[d] : Mb[5][d];
    }
    const uint32_t belowA = band_below(gIa[NPL - 1]), belowB = band_below(gIb[NPL - 1]);
    const uint32_t aboveA = band_above(gDa[0]), aboveB = band_above(gDb[0]);
    uint32_t pa[NPL], pb[NPL];
    bool term[NPL];
#pragma unroll
    for (int d = 0; d < NPL; ++d) {
      const int k = kA + d;
      const uint32_t kb = (uint32_t)(kbA + d);
      uint32_t ia = d ? gIa[d - 1] : belowA, ib = d ? gIb[d - 1] : belowB;                          // sources at k - 1
      uint32_t da = d < NPL - 1 ? gDa[d + 1] : aboveA, db = d < NPL - 1 ? gDb[d + 1] : aboveB;  // sources at k + 1
      ia += min(band_enc(ia), 1u);  // + 1 unless NULL
      // a gap cell at v <= 0 or h <= 0: the back-trace ends there, nothing of its path counts
      { const int hh = (int)band_enc(ia) - 1, vv = hh - k; if (hh <= 0 || vv <= 0) { ia &= 0xFFFFu; ib = 0u; } }
      { const int hh = (int)band_enc(da) - 1, vv = hh - k; if (hh <= 0 || vv <= 0) { da &= 0xFFFFu; db = 0u; } }
      Ia[d] = ia; Ib[d] = ib; Da[d] = da; Db[d] = db;
      // mismatch: M[s-2][k] + 1 and an X operation from (v - 1, h - 1) to (v, h)
      uint32_t xa = Ma[1][d], xb = Mb[1][d];
      if (band_enc(xa)) {
        xa += 1u;
        const uint32_t vv = band_enc(xa) - 1u - (uint32_t)k;
        if (!(xb & B_STARTED)) { xa = (xa & 0x00FFFFFFu) | ((vv - 1u) << 24); xb = (kb << 8) | B_STARTED; }
        xb = (xb & ~(B_PE | B_KL)) | vv | (kb << 17);
      }
      // the maximum wins; ties: mis > del > ins
      const bool dwin = band_enc(da) >= band_enc(ia);
      uint32_t qa = dwin ? da : ia, qb = dwin ? db : ib;
      const bool xwin = band_enc(xa) >= band_enc(qa);
      pa[d] = xwin ? xa : qa; pb[d] = xwin ? xb : qb;
      if (s == 0) { pa[d] = k >= 0 && k <= tbf ? (uint32_t)k + 1u : 0u; pb[d] = 0u; }
    }
    const bool t = extend_cells(pa, pb, term);
    trim(Ia, Ib); trim(Da, Db);
    terminated(s, t, pa, pb, term);
#pragma unroll
    for (int d = 0; d < NPL; ++d) {
#pragma unroll
      for (int r = 5; r >= 1; --r) { Ma[r][d] = Ma[r - 1][d]; Mb[r][d] = Mb[r - 1][d]; }
      Ma[0][d] = pa[d]; Mb[0][d] = pb[d];
    }
  }
  BandEnd E;
  E.s = end_s; E.a = end_a; E.b = end_b;
  return E;
}

// a job handed on to another list: piece and output slot from the record, the text and the band word as given, no CIGAR / operation slots
__device__ __forceinline__ void band_hand_on(JobDev* dst, const JobDev* src, uint64_t txt_off, uint32_t txt_len, uint32_t pad, uint32_t out_index) {
  dst->pat_off = src->pat_off; dst->txt_off = txt_off; dst->cigar_off = 0; dst->ops_off = 0;
  dst->pat_len = src->pat_len; dst->txt_len = txt_len; dst->out_index = out_index; dst->pad = pad;
}

__global__ void __launch_bounds__(64, 2) wfa_band_kernel(const BandKArgs a) {
  __shared__ uint32_t lds_seq[2 * BAND_SEQ_DW];
  uint32_t* const Pq = lds_seq;
  uint32_t* const Tq = lds_seq + BAND_SEQ_DW;
  const int lane = threadIdx.x;
  const uint32_t n_jobs = *a.n_jobs_dev;
  uint32_t n_taken = 0;
  for (;;) {
    uint32_t jc = 0;
    if (lane == 0) jc = atomicAdd(a.count + a.i_claim, 1u);  // one job per claim: job costs differ by 10x and more
    const uint32_t j = (uint32_t)band_rfl((int)jc);
    if (j >= n_jobs) break;
    // (the record field by field, here and where it is handed on: a local copy of it is an alloca, which the compiler moves to LDS)
    const JobDev* const job = a.jobs + j;
    const uint32_t pad = (uint32_t)band_rfl((int)job->pad), o = (uint32_t)band_rfl((int)job->out_index);
    const int plen = band_rfl((int)job->pat_len), rlen = band_rfl((int)job->txt_len);
    const int s_star = (int)((pad >> 16) & 0x7FFFu), k_end = (int)(pad & 0xFFFFu) - plen;
    const int t0 = max(0, k_end - s_star), k_hi = min(k_end + s_star, rlen), t_end = min(rlen, k_end + s_star + plen);
    if (!((pad >> 31) && s_star <= a.s_max && k_hi >= t0 && t_end > t0)) {  // no band for this job: the whole read
      if (lane == 0) band_hand_on(a.rest_jobs + atomicAdd(a.count + a.i_rest, 1u), job, job->txt_off, job->txt_len, 0u, o);
      continue;
    }
    if (s_star > BAND_CAP || plen > BAND_PLEN_MAX) {  // a band the layout does not hold: the LDS launch
      if (lane == 0) { JobDev* const dst = a.fall_jobs + atomicAdd(a.count + a.i_fall, 1u); band_hand_on(dst, job, job->txt_off, job->txt_len, pad, o); dst->cigar_off = job->cigar_off; dst->ops_off = job->ops_off; }
      continue;
    }
    ++n_taken;
    const int tlen = t_end - t0, tbf = k_hi - t0;
    band_stage(a.pat_base + job->pat_off, plen, Pq, lane);
    band_stage(a.txt_base + job->txt_off + (uint64_t)t0, tlen, Tq, lane);
    asm volatile("" ::: "memory");  // (one wave: LDS operations complete in order, nothing to wait for)

    // the band [-s*, tbf + s*] on the fewest diagonals per lane that hold it
    const int kbase = -s_star, width = tbf + 2 * s_star + 1;
    BandEnd E;
    if (width <= 128) E = band_run<2>(Pq, Tq, lane, plen, tlen, tbf, s_star, kbase);
    else if (width <= 256) E = band_run<4>(Pq, Tq, lane, plen, tlen, tbf, s_star, kbase);
    else if (width <= 384) E = band_run<6>(Pq, Tq, lane, plen, tlen, tbf, s_star, kbase);
    else E = band_run<BAND_NPL>(Pq, Tq, lane, plen, tlen, tbf, s_star, kbase);
    const int end_s = E.s; const uint32_t end_a = E.a, end_b = E.b;
    // ---- what band_check_kernel asked of the LDS launch: the pre-filter's penalty, and matches
    const int nm = (int)((end_a >> 16) & 0xFFu);
    if (lane == 0) {
      if (end_s == s_star && nm > 0) {
        const uint32_t ps = end_a >> 24, pe = end_b & B_PE;
        const int kf = (int)((end_b >> 8) & 0x1FFu) + kbase, kl = (int)((end_b >> 17) & 0x1FFu) + kbase;
        a.n_match[o] = nm;
        *reinterpret_cast<uint4*>(a.span4 + 4 * (size_t)o) = make_uint4(ps, pe, (uint32_t)((int)ps + kf + t0), (uint32_t)((int)pe + kl + t0));
      } else {
        a.n_match[o] = -1;
        band_hand_on(a.rest_jobs + atomicAdd(a.count + a.i_rest, 1u), job, a.read_off[o >> 1], a.read_len[o >> 1], 0u, o);  // against its whole read
        atomicAdd(a.count + a.i_fail, 1u);
      }
    }
  }
  if (lane == 0 && n_taken) atomicAdd(a.count + a.i_reg, n_taken);
}

}  // namespace

int wfa_band_launch(trgt_hip_ctx* c, const WfaBandLaunch& L) {
  BandKArgs a;
  a.jobs = L.jobs_dev; a.n_jobs_dev = L.n_jobs_dev; a.pat_base = L.pat_base; a.txt_base = L.txt_base;
  a.count = L.count; a.i_claim = L.i_claim; a.i_reg = L.i_reg; a.i_fall = L.i_fall; a.i_rest = L.i_rest; a.i_fail = L.i_fail;
  a.fall_jobs = L.fall_jobs; a.rest_jobs = L.rest_jobs; a.n_match = L.n_match; a.span4 = L.span4;
  a.read_off = L.read_off; a.read_len = L.read_len; a.s_max = L.s_max;
  // persistent one-wave workgroups, as many as can be resident; the number of jobs is known on the device only
  if (c->band_occ < 1) {  // (asked once per context: the answer depends on the kernel and the device only)
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, wfa_band_kernel, 64, 0) != hipSuccess || occ < 1) { (void)hipGetLastError(); occ = 8; }
    c->band_occ = std::min(occ, 16);
  }
  const int occ = c->band_occ;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)c->num_cus * occ, L.n_jobs_host));
  if (c->knobs.debug) fprintf(stderr, "[wfa] banded launch in registers: occupancy=%d grid=%lld\n", occ, (long long)grid);
  KTimer t(c, L.timer_slot);
  hipLaunchKernelGGL(wfa_band_kernel, dim3((unsigned)grid), dim3(64), 0, c->stream, a);
  TRGT_HIP_TRY(c, hipGetLastError());
  t.stop(0);
  return TRGT_OK;
}

}  // namespace trgt
