// trgt_amd/csrc/spans.hip -- trgt_find_spans_batch: locate the repeat inside every read.
//
// Replaces find_spans / find_tr_spans of PacificBiosciences/trgt v3.0.0
// (src/trgt/genotype/span_locater.rs:7-68): per read and per flank piece, the leftmost exact
// occurrence (windows().position(), :10-12), else a gap-affine ends-free wavefront alignment of the
// piece against the whole read (THREAD_WFA_FLANK, src/commands/genotype.rs:66-80; :14-26) accepted
// when count_matches() >= flank_len * min_flank_id_frac; the two flank hits are combined into the
// repeat span (:52-66).
//
// Launches on the ctx stream, no host round trip in between:
//   1. flank_scan_wide_kernel  one wavefront per read, both pieces at once: 1024 read bytes per round, 16 candidate
//                          windows per lane from one 24-byte load, 8-byte filter, cooperative verify in increasing
//                          position -> leftmost hit.  Misses are appended to a device-side job list (atomic counter).
//                          (flank_scan_kernel, one wavefront per (read, side), remains for flank_len < 4.)
//   2. wfa_fast_kernel     (wfa_fast.hpp) persistent workgroups drain that list: first the alignments of the reads too short to
//                          span their locus; then (flank_window_kernel, window_check_kernel) the other alignments on a seeded
//                          window of the read where one can be proven sufficient; then the rest against the whole read.
//   3. span_combine_kernel per read: threshold test and (lf.end, rf.start) combination.
#include <algorithm>
#include <cmath>
#include <optional>

#include "wfa_host.hpp"

namespace trgt {

// The counter block of a find_spans call (SC_WORDS words in HBM, cleared in front of the scan): list lengths and tallies shared by its kernels.
enum SpanCount : int {
  SC_HEAVY = 0,     // expensive fallback alignments: the front of the two-ended job list
  SC_LONG = 1,      // reads beyond the dedicated kernels' texts (second list)
  SC_LIGHT = 2,     // the other fallback alignments: the back of the two-ended list
  SC_ZERO = 3,      // stays 0 (the "front" count of a launch that takes the back of the list only)
  SC_WIN = 4,       // alignments on a seeded window
  SC_REST = 5,      // alignments against the whole read (no window, or a window that did not stand)
  SC_KEEP = 6,      // what the pre-filter keeps for the back-tracing launch
  SC_SHORTCUT = 7,  // alignments settled by the substitution / one-base-gap shortcuts
  SC_NOSEED = 8,    // expensive alignments without seeds inside the read: the pre-filter's list
  SC_GAPS = 9,      // of SC_SHORTCUT: one-base gaps
  SC_BAND = 10,     // of SC_KEEP: back-traced inside the band the pre-filter's penalty and end diagonal allow
  SC_HREST = 11,    // of SC_KEEP: the others (and the banded ones that did not stand), back-traced over the whole read
  SC_BANDFAIL = 12, // banded runs that did not come out with the pre-filter's penalty (the argument says: none)
  SC_LBAND = 13,    // long reads (SC_LONG) whose windows named the penalty and the end diagonal: back-traced inside a band
  SC_LREST = 14,    // ... the other long reads the window filter keeps: back-traced over the whole read
  SC_LNOSEED = 15,  // long reads' alignments the seed search could neither settle nor window (or whose window did not stand): the window filter's list
  SC_SIBDROP = 16,  // missed pieces the scan did not turn into a job: the exactly found sibling leaves them fewer than min_matches bases (ScanArgs::min_matches)
  SC_WINCLAIM = 17, // job claims of the register kernel over the windowed list (wfa_win.hip)
  SC_WINFALL = 18,  // windowed alignments that kernel did not take (sequences beyond its staging buffers): they go on to the whole-read launch
  SC_SETDROP = 19,  // of SC_NOSEED: jobs the pre-filter never sees, the sibling the shortcuts settled leaves them fewer than min_matches bases (settled_sibling_kernel)
  SC_FILTER = 20,   // ... the others: the pre-filter's list where that rule or the next is on
  SC_LCSDROP = 21,  // of SC_NOSEED: jobs the pre-filter never sees, their piece has no common subsequence of min_matches bases with the read beside a known sibling span (lcs_below)
  // the one-wave forward kernel over a kept list (wfa_band.hip); with it SC_BAND / SC_LBAND count only what the LDS launch behind it bands
  SC_BANDCLAIM = 22, // its job claims
  SC_BANDFALL = 23,  // banded jobs it leaves to the LDS launch (penalty or piece beyond its layout)
  SC_BANDREG = 24,   // of SC_KEEP: back-traced inside their band by it
  SC_LBANDCLAIM = 25, SC_LBANDFALL = 26, SC_LBANDREG = 27,  // the same three for the long reads' kept list
  SC_WORDS = 28
};

struct ScanArgs {
  const uint8_t* flank_blob; const uint8_t* read_blob;
  const uint64_t* piece_off;   // [2 * n_loci] left piece, right piece (offsets into flank_blob)
  const uint64_t* read_off; const uint32_t* read_len; const uint32_t* read_locus;
  uint64_t n_jobs;             // 2 * n_reads
  int32_t flank_len;
  int32_t* pos;                // [n_jobs] leftmost exact start or -1
  int32_t* n_match;            // [n_jobs] initialised to -1 here (the alignment kernels fill in the jobs they run)
  JobDev* wfa_jobs; uint32_t* wfa_count;  // fallback alignments: two-ended job list.  Reads shorter than heavy_len[locus] cannot hold
                                          // both flanks: their alignments run to high scores and cost 10-100x the others, so they
                                          // are appended from the front (wfa_count[0]) and drained first; the rest from the back
                                          // (wfa_jobs[jobs_cap - 1 - k], wfa_count[2]).  Longest-first keeps the tail of the
                                          // persistent alignment kernel short (12.45 vs 13.0 ms on the 10k-locus batch).
  const uint32_t* heavy_len; uint32_t jobs_cap;
  JobDev* wfa_jobs_long; uint32_t long_tlen;  // reads longer than long_tlen go to a second list (wfa_count[1]): they would not fit the
                                              // LDS budget of the dedicated kernel and must not drag the whole batch onto the generic one
  // > 0: the sibling rule of flank_scan_wide_kernel.  The reference combines the two flank hits of a read as (lf.end, rf.start) and
  // returns None when either is missing or lf.end > rf.start (span_locater.rs:52-66); nothing else of a flank alignment leaves
  // find_tr_spans.  With one piece found exactly and the other missed, the missed piece's alignment therefore counts only if its text
  // span lies on the far side of the sibling: inside [p0 + F, n) for a missed right piece (left found at p0), inside [0, p1) for a
  // missed left piece (right found at p1).  count_matches() cannot exceed the text span, so where that region holds fewer than
  // min_matches = ceil(flank_len * min_flank_id_frac) bases the read's span is None whatever the alignment is -- below the threshold
  // (:18-22) if it stays inside the region, discordant if it leaves it -- and no job is emitted.  The hit byte of such a piece reads 0
  // where the alignment might have made it 2: callers that hand the bytes out keep the rule off (find_spans_device, span_only).
  int32_t min_matches;
  uint8_t* settled;  // not NULL: [n_jobs] cleared here, one byte per (read, side); the front seed search marks what its shortcuts settle (SettledArgs)
};

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__global__ void __launch_bounds__(256) flank_scan_kernel(const ScanArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= a.n_jobs) return;  // whole wave exits together
  const int lane = threadIdx.x & 63;
  const uint64_t r = j >> 1;
  const int side = (int)(j & 1);
  const int F = a.flank_len, n = (int)a.read_len[r];
  const uint8_t* __restrict__ piece = a.flank_blob + a.piece_off[2 * (uint64_t)a.read_locus[r] + side];
  const uint8_t* __restrict__ read = a.read_blob + a.read_off[r];
  int found = -1;
  if (n >= F) {
    const int last = n - F;  // last candidate start
    const uint32_t head = F >= 4 ? load_u32(piece) : 0;
    for (int base = 0; base <= last && found < 0; base += 64) {
      const int p = base + lane;
      bool hit = false;
      if (p <= last) {
        hit = F < 4 || load_u32(read + p) == head;
        if (hit) {
          int i = F >= 4 ? 4 : 0;
          for (; i + 4 <= F; i += 4)
            if (load_u32(read + p + i) != load_u32(piece + i)) { hit = false; break; }
          if (hit)
            for (; i < F; ++i)
              if (read[p + i] != piece[i]) { hit = false; break; }
        }
      }
      const unsigned long long m = __ballot(hit);
      if (m) found = base + (__ffsll((long long)m) - 1);
    }
  }
  if (lane == 0) {
    a.pos[j] = found; a.n_match[j] = -1;
    if (a.settled) a.settled[j] = 0;
    if (found < 0) {  // fall back to the wavefront aligner (span_locater.rs:13-26)
      const bool lng = (uint32_t)n > a.long_tlen;
      const uint32_t slot = atomicAdd(a.wfa_count + (lng ? SC_LONG : SC_HEAVY), 1u);
      JobDev jd;
      jd.pat_off = a.piece_off[2 * (uint64_t)a.read_locus[r] + side]; jd.txt_off = a.read_off[r];
      jd.cigar_off = 0; jd.ops_off = 0; jd.pat_len = (uint32_t)F; jd.txt_len = (uint32_t)n; jd.out_index = (uint32_t)j; jd.pad = 0;
      (lng ? a.wfa_jobs_long : a.wfa_jobs)[slot] = jd;
    }
  }
}

// ---- Seeded windows for the fallback alignments (an implementation shortcut with identical results, checked after the fact) ----
// The ends-free alignment of a flank piece against a whole read keeps every diagonal of the read alive at every score level,
// although the alignment it ends up with sits on a handful of diagonals.  When the optimal penalty s* is small this is provable
// up front.  Cut the piece into win_m segments of win_q bases.  With the conditions checked by window_plan() every mismatch or gap
// spoils at most as many segments as its penalty / x, so an alignment of penalty <= S0 = x * win_m - 1 leaves at least one segment
// matched exactly and gap-free: an exact occurrence of that segment at read position t pins the alignment to the diagonal
// k = t - (segment offset), and its path strays from k by at most G = (S0 - o) / e diagonals (its total gap length).  A wavefront
// cell (s, k) depends only on cells (s', k') with |k' - k| <= (s - s') / e.  So the alignment of the piece against the read window
// [kmin - G - C, kmax + G + C + F), C = S0 / e, kmin / kmax over ALL exact segment occurrences in the read, computes every cell the
// full run's termination test and back-trace would read -- bit for bit -- PROVIDED its penalty turns out <= S0 (window_check_kernel;
// otherwise, or when the occurrences are spread too widely or there are none, the whole read is aligned as before).  Offsets of a
// windowed run never exceed those of the full run (fewer sources under the max), so it cannot end early either.
// One wavefront; kmin / kmax are wave-uniform scalars (kmin > kmax: no occurrence).
constexpr int WIN_SEGMENTS_DEFAULT = 8;  // (4, 6 and 8 are instantiated; TRGT_WIN_SEGMENTS picks another one.  Measured on the 10k-locus
                                         // batch, search + alignments: 4 -> 3.19 ms, 6 -> 3.00, 8 -> 2.90, 10 -> 2.97, 12 -> 3.02)
// An "occurrence" is a match of the first TWELVE bases of a segment (all from registers: no memory round trip per candidate).  That
// is a superset of the exact occurrences, which is all the argument needs -- a chance match (4^-12 per position) can only widen
// the window or make the spread test fail.
template <int WIN_SEGMENTS>
__device__ __forceinline__ void piece_window_heads(const uint8_t* __restrict__ read, int n, const uint64_t (&h)[WIN_SEGMENTS], const uint32_t (&h3)[WIN_SEGMENTS], int q, int lane,
                                                   int& kmin_out, int& kmax_out);
template <int WIN_SEGMENTS>
__device__ __forceinline__ void piece_window(const uint8_t* __restrict__ read, int n, const uint8_t* __restrict__ piece, int q, int lane,
                                             int& kmin_out, int& kmax_out) {
  uint64_t h[WIN_SEGMENTS]; uint32_t h3[WIN_SEGMENTS];
#pragma unroll
  for (int i = 0; i < WIN_SEGMENTS; ++i) {  // (all loads in flight together)
    const uint8_t* __restrict__ seg = piece + i * q;
    h[i] = (uint64_t)load_u32(seg + 4) << 32 | load_u32(seg);
    h3[i] = load_u32(seg + 8);
  }
  piece_window_heads<WIN_SEGMENTS>(read, n, h, h3, q, lane, kmin_out, kmax_out);
}
// ... with the twelve head bytes of every segment already in registers (flank_window_kernel fetches them for all jobs of a wave up front)
template <int WIN_SEGMENTS>
__device__ __forceinline__ void piece_window_heads(const uint8_t* __restrict__ read, int n, const uint64_t (&h)[WIN_SEGMENTS], const uint32_t (&h3)[WIN_SEGMENTS], int q, int lane,
                                                   int& kmin_out, int& kmax_out) {
  int kmin = 0x7FFFFFFF, kmax = -0x7FFFFFFF;
  const int last = n - 12;  // last start of a twelve-base match
  for (int base = 0; base <= last; base += 1024) {
    const int off = base + 16 * lane;
    uint32_t w[7] = {0, 0, 0, 0, 0, 0, 0};
    if (off + 28 <= n) {
      uint4 v; uint2 v2; uint32_t v3;
      __builtin_memcpy(&v, read + off, 16); __builtin_memcpy(&v2, read + off + 16, 8); __builtin_memcpy(&v3, read + off + 24, 4);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; w[4] = v2.x; w[5] = v2.y; w[6] = v3;
    } else if (off < n) {
      // the lane that crosses the end of the read (the whole wave walks this branch with it): whole dwords while they fit, then the last
      // one to three bytes out of the dword that ENDS with the read -- seven independent loads and a shift (byte by byte it was 28
      // dependent iterations, a fifth of the kernel's instructions)
      const int rem = n - off, full = rem >> 2, tail = rem & 3;
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (k < full) w[k] = load_u32(read + off + 4 * k);
      if (tail && full < 7) {
        const uint32_t t = n >= 4 ? load_u32(read + n - 4) >> (8 * (4 - tail)) : 0u;  // bytes n - tail .. n - 1, zero above
        if (n >= 4) {
#pragma unroll
          for (int k = 0; k < 7; ++k) if (k == full) w[k] = t;
        } else {
          for (int b = 4 * full; b < rem; ++b) w[b >> 2] |= (uint32_t)read[off + b] << (8 * (b & 3));
        }
      }
    }
    // The first FOUR bytes at every candidate start decide whether a segment is looked at more closely in this round: a 32-bit
    // compare per position and segment, kept as a BALLOT (the compares land in SGPR pairs anyway).  Everything behind it is uniform
    // over the wave: the segment is skipped when no lane has a candidate, and of its sixteen positions only those where some lane
    // has one are verified -- a scalar compare and branch each -- against the other eight bytes, lo[s16 + 4] and lo[s16 + 8] of the
    // 24 candidate dwords formed once per round.  The verified matches are balloted again; their lowest and highest lane give the
    // smallest and largest position of that s16 (a flank of period 16, 8, 4, 2 or 1 has several lanes there, one ballot takes them
    // all), so kmin / kmax are scalars and nothing is reduced across lanes at the end.  With per-lane branches every seeded
    // segment verified all sixteen positions in every lane (about 75 vector instructions, four of the bodies if-converted and
    // unconditional), and a six-step butterfly over kmin / kmax followed (46 more, twelve LDS round trips per job): 1 234 vector
    // instructions per job then, 659 now -- for 9 % of the kernel's time, the rest is the job's chain of loads and scalar work
    // (DESIGN.md section 5).  The compiler flattens a uniform `if` whose body it can speculate -- a plain `if (m[s16] != 0)` had
    // all sixteen bodies if-converted, 175 vector instructions per segment -- so each body begins with an empty `asm volatile`,
    // which keeps the branch (as in wfa_band.hip; read the listing after a change: about 22 vector instructions per seeded segment).
    uint32_t lo[24];
#pragma unroll
    for (int j = 0; j < 24; ++j) {
      const int d = j >> 2, sh = j & 3;
      lo[j] = sh == 0 ? w[d] : __builtin_amdgcn_alignbyte(w[d + 1], w[d], sh);
    }
#pragma unroll
    for (int i = 0; i < WIN_SEGMENTS; ++i) {
      const uint32_t h_lo = (uint32_t)h[i], h_hi = (uint32_t)(h[i] >> 32);
      unsigned long long m[16], any = 0ull;
#pragma unroll
      for (int s16 = 0; s16 < 16; ++s16) { m[s16] = __ballot(lo[s16] == h_lo); any |= m[s16]; }
      if (any == 0ull) continue;  // (taken but for the round that holds an occurrence of this segment, or four of its bases by chance)
#pragma unroll
      for (int s16 = 0; s16 < 16; ++s16) {
        if (m[s16] != 0ull) {
          asm volatile("" ::: "memory");  // (not speculatable: the branch stays a branch)
          const unsigned long long full = m[s16] & __ballot(lo[s16 + 4] == h_hi && lo[s16 + 8] == h3[i] && off + s16 <= last);
          if (full != 0ull) {
            const int k0 = base + s16 - i * q;
            const int k_lo = k0 + 16 * (int)__builtin_ctzll(full), k_hi = k0 + 16 * (63 - (int)__builtin_clzll(full));
            kmin = k_lo < kmin ? k_lo : kmin; kmax = k_hi > kmax ? k_hi : kmax;
          }
        }
      }
    }
  }
  kmin_out = kmin; kmax_out = kmax;
}

// One wavefront per fallback alignment of the light list (the back of wfa_jobs): jobs that get a window go to win_jobs (count[4],
// JobDev::pad = first text base of the window), the others to rest_jobs (count[5]).  A workgroup takes WIN_JOBS_PER_WG jobs and
// reserves its output slots with one atomic per list.
struct WindowArgs {
  const uint8_t* flank_blob; const uint8_t* read_blob;
  const JobDev* wfa_jobs; uint32_t jobs_cap; uint32_t* count;
  JobDev* win_jobs; JobDev* rest_jobs;
  int32_t flank_len, q, margin, spread, tbf;
  int32_t front;                       // 1: the jobs at the FRONT of wfa_jobs (count[0], the expensive ones); the jobs without a window then go to rest_jobs under count[8]
  const JobDev* long_jobs; JobDev* long_rest;  // not NULL (with front == 0): the long reads' list (count[SC_LONG]) behind the light one; its jobs without a window go to long_rest under count[SC_LNOSEED]
  int32_t hamming_max;                 // > 0: the substitution-only shortcut below, for up to this many mismatches
  int32_t indel_ok;                    // 1: the one-base-gap shortcut (penalties 2,5,1)
  int32_t* n_match; uint32_t* span4;   // per (read, side): what the alignment kernels would have written for such a job
  uint8_t* settled;                    // not NULL: per (read, side), set to 1 where a shortcut wrote them (the scan cleared it)
};
constexpr int WIN_JOBS_PER_WG = 64;
template <int WIN_SEGMENTS>
__global__ void __launch_bounds__(256) flank_window_kernel(const WindowArgs a) {
  __shared__ JobDev l_out[WIN_JOBS_PER_WG];  // windowed jobs from the front, the others from the back
  __shared__ JobDev l_long[WIN_JOBS_PER_WG]; // long reads' jobs without a window
  __shared__ uint32_t l_nw, l_nr, l_bw, l_br, l_ns, l_ni, l_nl, l_bl;
  // (the length of the list this launch walks; with long_jobs the long reads' list behind it -- ONE launch: a second one would wait behind the
  //  pre-filter's persistent workgroups of the other stream, 1.6 ms for 9 k jobs on the catalog mix)
  const uint32_t n_first = a.count[a.front ? SC_HEAVY : SC_LIGHT], n_light = n_first + (a.long_jobs ? a.count[SC_LONG] : 0u);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // jobs per workgroup and round: 64, fewer when the list is short (a job is a dependent chain of loads: 17 k jobs in rounds of 64 kept
  // 270 workgroups busy for 0.39 ms; spread over all of them they take a fifth of that)
  const uint32_t per_wg = min((uint32_t)WIN_JOBS_PER_WG, max(4u, ((n_light + gridDim.x - 1u) / gridDim.x + 3u) & ~3u));
  for (uint32_t c0 = blockIdx.x * per_wg; c0 < n_light; c0 += gridDim.x * per_wg) {
    if (threadIdx.x == 0) { l_nw = 0; l_nr = 0; l_ns = 0; l_ni = 0; l_nl = 0; }
    __syncthreads();
    const uint32_t c1 = c0 + per_wg < n_light ? c0 + per_wg : n_light;
    // (a job is a chain of dependent loads -- the job, the heads of its piece's segments, the read -- and a wave walks up to sixteen of
    //  them: lane j fetches the first two links for the wave's j-th job up front, as the scan does, round 5)
    uint64_t pf_pat = 0, pf_txt = 0, pf_cig = 0, pf_ops = 0;
    uint32_t pf_plen = 0, pf_tlen = 0, pf_oi = 0, pf_pad = 0, pf_hlo[WIN_SEGMENTS], pf_hhi[WIN_SEGMENTS], pf_h3[WIN_SEGMENTS];
#pragma unroll
    for (int sg = 0; sg < WIN_SEGMENTS; ++sg) { pf_hlo[sg] = 0; pf_hhi[sg] = 0; pf_h3[sg] = 0; }
    {
      const uint32_t ij = c0 + (uint32_t)wave + 4u * (uint32_t)lane;
      if (lane < WIN_JOBS_PER_WG / 4 && ij < c1) {
        const JobDev pj = ij >= n_first ? a.long_jobs[ij - n_first] : a.front ? a.wfa_jobs[ij] : a.wfa_jobs[a.jobs_cap - 1u - ij];
        pf_pat = pj.pat_off; pf_txt = pj.txt_off; pf_cig = pj.cigar_off; pf_ops = pj.ops_off; pf_plen = pj.pat_len; pf_tlen = pj.txt_len; pf_oi = pj.out_index; pf_pad = pj.pad;
        if (pj.txt_len >= 12u) {
#pragma unroll
          for (int sg = 0; sg < WIN_SEGMENTS; ++sg) {
            const uint8_t* __restrict__ seg = a.flank_blob + pj.pat_off + sg * a.q;
            pf_hlo[sg] = load_u32(seg); pf_hhi[sg] = load_u32(seg + 4); pf_h3[sg] = load_u32(seg + 8);
          }
        }
      }
    }
    auto lane32 = [](uint32_t v, int j) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); };
    auto lane64 = [&](uint64_t v, int j) -> uint64_t { return (uint64_t)lane32((uint32_t)v, j) | ((uint64_t)lane32((uint32_t)(v >> 32), j) << 32); };
    int slot = 0;
    for (uint32_t i = c0 + (uint32_t)wave; i < c1; i += 4, ++slot) {
      const bool is_long = i >= n_first;
      JobDev jd;
      jd.pat_off = lane64(pf_pat, slot); jd.txt_off = lane64(pf_txt, slot); jd.cigar_off = lane64(pf_cig, slot); jd.ops_off = lane64(pf_ops, slot);
      jd.pat_len = lane32(pf_plen, slot); jd.txt_len = lane32(pf_tlen, slot); jd.out_index = lane32(pf_oi, slot); jd.pad = lane32(pf_pad, slot);
      const int n = (int)jd.txt_len, F = a.flank_len;
      int kmin = 1, kmax = 0;
      if (n >= 12) {
        uint64_t h[WIN_SEGMENTS]; uint32_t h3[WIN_SEGMENTS];
#pragma unroll
        for (int sg = 0; sg < WIN_SEGMENTS; ++sg) { h[sg] = (uint64_t)lane32(pf_hlo[sg], slot) | ((uint64_t)lane32(pf_hhi[sg], slot) << 32); h3[sg] = lane32(pf_h3[sg], slot); }
        piece_window_heads<WIN_SEGMENTS>(a.read_blob + jd.txt_off, n, h, h3, a.q, lane, kmin, kmax);
      }
      // ---- The alignment of a piece that differs from the read by one or two substitutions, without aligning.  All seeds on ONE
      //      diagonal k with the piece inside the read there, d <= hamming_max = min(segments - 1, (o + e - 1) / x, 4) mismatches on it:
      //      every alignment of penalty <= x d < o + e is gap-free, i.e. a diagonal k' with at most d mismatches; those spoil at most
      //      d segments, the others occur exactly on k' and their heads are among the seeds, so k' = k.  The optimal alignment is
      //      therefore unique -- diagonal k, penalty x d -- and what the reference reads off it (span_locater.rs:14-26) is
      //      count_matches() = F - d and the text span [k, k + F).  (d = 0 cannot happen: the exact scan would have found it.)
      bool solved = false;
      if (a.hamming_max > 0 && kmin == kmax && kmin >= 0 && kmin + F <= n) {
        const uint8_t* __restrict__ t = a.read_blob + jd.txt_off + kmin;
        const uint8_t* __restrict__ pz = a.flank_blob + jd.pat_off;
        auto differing_bytes = [](uint32_t x) -> uint32_t { return (uint32_t)__builtin_popcount((x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u); };
        uint32_t cnt = 0;
        for (int i = lane; i < (F >> 2); i += 64) cnt += differing_bytes(load_u32(t + 4 * i) ^ load_u32(pz + 4 * i));
        if (lane == 63 && (F & 3)) cnt += differing_bytes((load_u32(t + F - 4) ^ load_u32(pz + F - 4)) >> (8 * (4 - (F & 3))));  // the last one to three bytes
        // (the sum over the lanes from four ballots: a shuffle reduction is six LDS round trips per job, as much as the search itself)
        const unsigned long long b1 = __ballot(cnt >= 1u);
        uint32_t total = (uint32_t)__popcll(b1);
        if (total <= (uint32_t)a.hamming_max) total += (uint32_t)(__popcll(__ballot(cnt >= 2u)) + __popcll(__ballot(cnt >= 3u)) + __popcll(__ballot(cnt >= 4u)) + __popcll(__ballot(cnt >= 5u)));
        cnt = total;  // (uniform; lanes hold at most one dword and the tail for flanks up to 255 bases, more only beyond -- then cnt >= 5 ends the shortcut)
        if (cnt >= 1u && cnt <= (uint32_t)a.hamming_max) {
          solved = true;
          if (lane == 0) {
            const uint64_t j = jd.out_index;
            a.n_match[j] = F - (int)cnt;
            a.span4[4 * j] = 0u; a.span4[4 * j + 1] = (uint32_t)F; a.span4[4 * j + 2] = (uint32_t)kmin; a.span4[4 * j + 3] = (uint32_t)(kmin + F);
            if (a.settled) a.settled[j] = 1;
            atomicAdd(&l_ns, 1u);  // (one global atomic per workgroup below: 60k of them on one address doubled this kernel's time)
          }
        }
      }
      // ---- ... and of a piece that differs from the read by ONE inserted or deleted base (penalties 2,5,1 only: o + e = 6).  All seeds on
      //      two neighbouring diagonals, both inside the read.  An alignment of penalty <= 6 is gap-free with <= 3 mismatches, or has one
      //      gap of one base and no mismatch.  The former leaves five segments exact, so it lies on a seeded diagonal: excluded when both
      //      have >= 4 mismatches -- and with 2 and 4 excluded as well, the optimal penalty is 6.  The latter leaves seven segments exact;
      //      the part on either side of the gap that holds a whole segment head lies on a seeded diagonal.  Both parts seeded: prefix on
      //      one, suffix on the other of the two diagonals -- feasible iff the exact prefix on the first reaches the exact suffix on the
      //      second (lcp / sfx below), and required to be feasible in ONE order only.  One part without a head (fewer than 12 bases in
      //      front of the gap, or a suffix that starts beyond the last head): then the other part is exact from within 13 bases of the
      //      start, or up to the last head, on a seeded diagonal -- excluded by the two margin tests.  So every optimal alignment runs
      //      along the first diagonal, takes the one-base gap somewhere in the overlap of prefix and suffix (a homopolymer leaves the
      //      place open, nothing else) and ends on the second: count_matches() and the span are the same for all of them --
      //      F matches over F + 1 bases for an inserted base, F - 1 over F - 1 for a deleted one (span_locater.rs:14-26).
      if (!solved && a.indel_ok && kmax - kmin == 1 && kmin >= 0 && kmax + F <= n && F <= 255) {
        const uint8_t* __restrict__ t = a.read_blob + jd.txt_off + kmin;
        const uint8_t* __restrict__ pz = a.flank_blob + jd.pat_off;
        const int nd = F >> 2, rem = F & 3;
        uint32_t pw = 0, t0 = 0, t1 = 0;  // lane i: bytes 4 i .. 4 i + 3 of the piece and of the read on the two diagonals; lane nd: the last one to three
        if (lane < nd) { pw = load_u32(pz + 4 * lane); t0 = load_u32(t + 4 * lane); t1 = load_u32(t + 1 + 4 * lane); }
        else if (lane == nd && rem) { const int sh = 8 * (4 - rem); pw = load_u32(pz + F - 4) >> sh; t0 = load_u32(t + F - 4) >> sh; t1 = load_u32(t + 1 + F - 4) >> sh; }
        auto byte_flags = [](uint32_t x) -> uint32_t { return (x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u; };  // bit 8 b + 7: byte b differs
        const uint32_t m0 = byte_flags(pw ^ t0), m1 = byte_flags(pw ^ t1);
        const unsigned long long b0 = __ballot(m0 != 0u), b1 = __ballot(m1 != 0u);
        auto lcp = [&](unsigned long long b, uint32_t m) -> int {  // bases of the piece that match from its start
          if (!b) return F;
          const int l = (int)__builtin_ctzll(b);
          return 4 * l + (__builtin_ctz((uint32_t)__builtin_amdgcn_readlane((int)m, l)) >> 3);
        };
        auto sfx = [&](unsigned long long b, uint32_t m) -> int {  // first base of the piece's exact suffix
          if (!b) return 0;
          const int l = 63 - (int)__builtin_clzll(b);
          return 4 * l + ((31 - __builtin_clz((uint32_t)__builtin_amdgcn_readlane((int)m, l))) >> 3) + 1;
        };
        auto at_least_4 = [&](unsigned long long b, uint32_t m) -> bool {  // mismatches on the diagonal
          const int lanes = __popcll(b);
          if (lanes >= 4) return true;
          const uint32_t c = (uint32_t)__builtin_popcount(m);
          return lanes + __popcll(__ballot(c >= 2u)) + __popcll(__ballot(c >= 3u)) + __popcll(__ballot(c >= 4u)) >= 4;
        };
        const int lcp0 = lcp(b0, m0), lcp1 = lcp(b1, m1), sfx0 = sfx(b0, m0), sfx1 = sfx(b1, m1);
        const int last_head = (WIN_SEGMENTS - 1) * a.q;
        const bool margins = sfx0 > 13 && sfx1 > 13 && lcp0 < last_head - 1 && lcp1 < last_head - 1;
        const bool ins_ok = sfx1 <= lcp0;                                  // prefix on kmin, one read base skipped, suffix on kmin + 1
        const bool del_ok = max(sfx0 - 1, 0) <= min(lcp1, F - 1);          // prefix on kmin + 1, one base of the piece skipped, suffix on kmin
        if (margins && ins_ok != del_ok && at_least_4(b0, m0) && at_least_4(b1, m1)) {
          solved = true;
          if (lane == 0) {
            const uint64_t j = jd.out_index;
            const int start = ins_ok ? kmin : kmax, len = ins_ok ? F + 1 : F - 1;
            a.n_match[j] = ins_ok ? F : F - 1;
            a.span4[4 * j] = 0u; a.span4[4 * j + 1] = (uint32_t)F; a.span4[4 * j + 2] = (uint32_t)start; a.span4[4 * j + 3] = (uint32_t)(start + len);
            if (a.settled) a.settled[j] = 1;
            atomicAdd(&l_ns, 1u);
            atomicAdd(&l_ni, 1u);
          }
        }
      }
      if (solved) continue;
      int w0 = 0, wl = 0;
      // (front list: only a piece that lies inside the read whole.  A read that ends within the piece has seeds too, but its alignment
      //  deletes the rest of the piece -- far beyond the bound of the window argument: it would fail the check and be aligned against
      //  the whole read without the pre-filter in front; measured, that put 6 ms of alignments behind a 1.4-ms filter pass)
      if (kmin <= kmax && kmax - kmin <= a.spread && (!a.front || (kmin >= 0 && kmax + F <= n))) {
        // diagonals [kmin - margin, kmax + margin] start the alignment (text_begin_free = 2 margin + spread of the windowed launch, counted
        // from the window start) and run through at most flank_len more bases of the read
        const int lo = kmin - a.margin;
        w0 = lo > 0 ? lo : 0;
        wl = n - w0 < a.tbf + F ? n - w0 : a.tbf + F;
      }
      if (lane == 0) {
        if (wl > 0) { jd.txt_off += (uint64_t)w0; jd.txt_len = (uint32_t)wl; jd.pad = (uint32_t)w0; l_out[atomicAdd(&l_nw, 1u)] = jd; }
        else if (is_long) l_long[atomicAdd(&l_nl, 1u)] = jd;
        else l_out[WIN_JOBS_PER_WG - 1 - atomicAdd(&l_nr, 1u)] = jd;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && l_nw) l_bw = atomicAdd(a.count + SC_WIN, l_nw);
    if (threadIdx.x == 64 && l_nr) l_br = atomicAdd(a.count + (a.front ? SC_NOSEED : SC_REST), l_nr);
    if (threadIdx.x == 65 && l_nl) l_bl = atomicAdd(a.count + SC_LNOSEED, l_nl);
    if (threadIdx.x == 128 && l_ns) atomicAdd(a.count + SC_SHORTCUT, l_ns);
    if (threadIdx.x == 192 && l_ni) atomicAdd(a.count + SC_GAPS, l_ni);  // (of those: one-base gaps)
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < l_nw; i += blockDim.x) a.win_jobs[l_bw + i] = l_out[i];
    for (uint32_t i = threadIdx.x; i < l_nr; i += blockDim.x) a.rest_jobs[l_br + i] = l_out[WIN_JOBS_PER_WG - 1 - i];
    for (uint32_t i = threadIdx.x; i < l_nl; i += blockDim.x) a.long_rest[l_bl + i] = l_long[i];
    __syncthreads();
  }
}

// One wavefront per READ, both flank pieces at once (flank_len >= 4).  A round covers 1024 read bytes: every lane loads 24
// consecutive bytes (16 + 8 of overlap), forms its 16 candidate windows with byte-align shifts and compares each with the first
// EIGHT bytes of the two pieces (four bases match by chance once in 256 positions: four false candidates per piece and read, each a
// dependent round trip to verify -- most of this kernel's time; eight bases: one in 65536); candidates are then verified in
// increasing position, cooperatively (lane i compares dword i of
// the piece), so the first full match is the leftmost occurrence, exactly windows().position() (span_locater.rs:10-12).
// A workgroup walks SCAN_READS_PER_WG reads (one per wave at a time) and collects its fallback jobs in LDS; one global atomic
// per workgroup reserves their slots in the job list (a per-job atomic on a single counter was most of this kernel's time).
constexpr int SCAN_READS_PER_WG = 64;
__global__ void __launch_bounds__(256) flank_scan_wide_kernel(const ScanArgs a) {
  __shared__ JobDev l_jobs[2 * SCAN_READS_PER_WG];  // expensive jobs fill it from the front, the others from the back
  __shared__ uint32_t l_n, l_n2, l_base, l_base2, l_drop;
  if (threadIdx.x == 0) { l_n = 0; l_n2 = 0; l_drop = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint64_t n_reads = a.n_jobs >> 1;
  const uint64_t r_begin = (uint64_t)blockIdx.x * SCAN_READS_PER_WG, r_end = r_begin + SCAN_READS_PER_WG < n_reads ? r_begin + SCAN_READS_PER_WG : n_reads;
  // What a read's search needs before its first byte can be looked at -- length, offset, locus, the locus' two piece offsets, the
  // pieces' first eight bytes -- is a chain of four dependent loads, and with one read at a time per wave that chain (not instruction
  // issue, not bandwidth) was most of this kernel's time: 300 k reads x ~5 us / 4 k resident waves.  Round 5: lane j fetches it all for
  // the wave's j-th read up front (four rounds of loads per wave instead of per read); the loop takes it from that lane.
  const int F = a.flank_len;
  const bool h8 = F >= 8;
  uint32_t pf_n = 0, pf_h0 = 0, pf_h1 = 0, pf_h20 = 0, pf_h21 = 0, pf_heavy = 0;
  uint64_t pf_roff = 0, pf_po0 = 0, pf_po1 = 0;
  {
    const uint64_t rj = r_begin + (threadIdx.x >> 6) + 4ull * (uint64_t)lane;
    if (lane < SCAN_READS_PER_WG / 4 && rj < r_end) {
      pf_n = a.read_len[rj]; pf_roff = a.read_off[rj];
      const uint64_t loc = a.read_locus[rj];
      pf_po0 = a.piece_off[2 * loc]; pf_po1 = a.piece_off[2 * loc + 1];
      if (a.heavy_len) pf_heavy = a.heavy_len[loc];
      if ((int)pf_n >= F) {
        pf_h0 = load_u32(a.flank_blob + pf_po0); pf_h1 = load_u32(a.flank_blob + pf_po1);
        if (h8) { pf_h20 = load_u32(a.flank_blob + pf_po0 + 4); pf_h21 = load_u32(a.flank_blob + pf_po1 + 4); }
      }
    }
  }
  auto from_lane32 = [](uint32_t v, int j) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); };
  auto from_lane64 = [&](uint64_t v, int j) -> uint64_t { return (uint64_t)from_lane32((uint32_t)v, j) | ((uint64_t)from_lane32((uint32_t)(v >> 32), j) << 32); };
  int slot = 0;
  for (uint64_t r = r_begin + (threadIdx.x >> 6); r < r_end; r += 4, ++slot) {
  const int n = (int)from_lane32(pf_n, slot);
  const uint64_t po0 = from_lane64(pf_po0, slot), po1 = from_lane64(pf_po1, slot);
  const uint8_t* __restrict__ piece[2] = {a.flank_blob + po0, a.flank_blob + po1};
  const uint64_t r_off = from_lane64(pf_roff, slot);
  const uint32_t heavy_r = from_lane32(pf_heavy, slot);
  const uint8_t* __restrict__ read = a.read_blob + r_off;
  int found[2] = {-1, -1};
  if (n >= F) {
    const int last = n - F;  // last candidate start
    const uint32_t head[2] = {from_lane32(pf_h0, slot), from_lane32(pf_h1, slot)};
    const uint32_t head2[2] = {from_lane32(pf_h20, slot), from_lane32(pf_h21, slot)};
    const int nd = F >> 2;   // full dwords of a piece
    for (int base = 0; base <= last && (found[0] < 0 || found[1] < 0); base += 1024) {
      const int off = base + 16 * lane;
      uint32_t w[6] = {0, 0, 0, 0, 0, 0};
      if (off + 24 <= n) {
        uint4 q; uint2 q2;
        __builtin_memcpy(&q, read + off, 16); __builtin_memcpy(&q2, read + off + 16, 8);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; w[4] = q2.x; w[5] = q2.y;
      } else if (off <= last) {
        // (a lane whose 24 bytes cross the end of the read AND that still holds a candidate start: only with pieces shorter than 24
        //  bases.  With TRGT's 250 the lanes at the end of a read start beyond the last candidate, their bytes are never looked at --
        //  and this byte loop, which the whole wave walks when one lane enters it, was a third of the kernel's instructions)
        for (int b = 0; b < 24 && off + b < n; ++b) w[b >> 2] |= (uint32_t)read[off + b] << (8 * (b & 3));
      }
      uint32_t m[2] = {0, 0};  // bit s: candidate start off + s matches the head of piece 0 / 1
      // (eight head bytes as one 64-bit compare per position and piece; the positions beyond the last candidate start are masked once
      //  per round, not tested per position: this kernel is bound by instruction issue)
      const uint64_t h64[2] = {(uint64_t)head[0] | ((uint64_t)head2[0] << 32), (uint64_t)head[1] | ((uint64_t)head2[1] << 32)};
#pragma unroll
      for (int s16 = 0; s16 < 16; ++s16) {
        const uint32_t win = (s16 & 3) == 0 ? w[s16 >> 2] : __builtin_amdgcn_alignbyte(w[(s16 >> 2) + 1], w[s16 >> 2], s16 & 3);
        if (h8) {
          const uint32_t win2 = (s16 & 3) == 0 ? w[(s16 >> 2) + 1] : __builtin_amdgcn_alignbyte(w[(s16 >> 2) + 2], w[(s16 >> 2) + 1], s16 & 3);
          const uint64_t w64 = (uint64_t)win | ((uint64_t)win2 << 32);
          m[0] |= (uint32_t)(w64 == h64[0]) << s16;
          m[1] |= (uint32_t)(w64 == h64[1]) << s16;
        } else {
          m[0] |= (uint32_t)(win == head[0]) << s16;
          m[1] |= (uint32_t)(win == head[1]) << s16;
        }
      }
      {
        const int room = last - off;  // candidate starts off .. off + room are inside the read
        const uint32_t vmask = room >= 15 ? 0xFFFFu : room < 0 ? 0u : (1u << (room + 1)) - 1u;
        m[0] &= vmask; m[1] &= vmask;
      }
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (found[side] >= 0) continue;
        uint32_t mm = m[side];
        for (;;) {
          const unsigned long long lanes = __ballot(mm != 0u);
          if (!lanes) break;
          const int lq = __ffsll((long long)lanes) - 1;
          const uint32_t mq = (uint32_t)__builtin_amdgcn_readlane((int)mm, lq);
          const int sq = __ffs((int)mq) - 1;
          const int p = base + 16 * lq + sq;
          bool ok = true;  // lane i verifies dwords i, i + 64, ... and the last lane the tail bytes
          for (int i = lane; i < nd; i += 64) ok = ok && load_u32(read + p + 4 * i) == load_u32(piece[side] + 4 * i);
          if (lane == 63 && (F & 3)) ok = ok && load_u32(read + p + F - 4) == load_u32(piece[side] + F - 4);  // the last one to three bytes: the dword that ends the piece (F >= 4)
          if (__ballot(!ok) == 0ull) { found[side] = p; break; }
          if (lane == lq) mm &= mm - 1u;  // drop this candidate
        }
      }
    }
  }
  if (lane == 0) {
    for (int side = 0; side < 2; ++side) {
      const uint64_t j = 2 * r + side;
      a.pos[j] = found[side]; a.n_match[j] = -1;
      if (a.settled) a.settled[j] = 0;
      // (ScanArgs::min_matches) what the exactly found sibling leaves this piece: the read behind the left piece, or in front of the right one
      const int room = found[side ^ 1] < 0 ? 0x7FFFFFFF : side ? n - found[0] - F : found[1];
      if (found[side] < 0 && room < a.min_matches) atomicAdd(&l_drop, 1u);
      else if (found[side] < 0) {  // fall back to the wavefront aligner (span_locater.rs:13-26)
        JobDev jd;
        jd.pat_off = side ? po1 : po0; jd.txt_off = r_off;
        jd.cigar_off = 0; jd.ops_off = 0; jd.pat_len = (uint32_t)F; jd.txt_len = (uint32_t)n; jd.out_index = (uint32_t)j; jd.pad = 0;
        if ((uint32_t)n > a.long_tlen) a.wfa_jobs_long[atomicAdd(a.wfa_count + SC_LONG, 1u)] = jd;  // rare: straight to the second list
        else if (!a.heavy_len || (uint32_t)n < heavy_r) l_jobs[atomicAdd(&l_n, 1u)] = jd;
        else l_jobs[2 * SCAN_READS_PER_WG - 1 - atomicAdd(&l_n2, 1u)] = jd;
      }
    }
  }
  }  // reads of this workgroup
  __syncthreads();
  if (threadIdx.x == 0 && l_n) l_base = atomicAdd(a.wfa_count + SC_HEAVY, l_n);
  if (threadIdx.x == 64 && l_n2) l_base2 = atomicAdd(a.wfa_count + SC_LIGHT, l_n2);
  if (threadIdx.x == 128 && l_drop) atomicAdd(a.wfa_count + SC_SIBDROP, l_drop);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < l_n; i += blockDim.x) a.wfa_jobs[l_base + i] = l_jobs[i];
  for (uint32_t i = threadIdx.x; i < l_n2; i += blockDim.x) a.wfa_jobs[a.jobs_cap - 1u - (l_base2 + i)] = l_jobs[2 * SCAN_READS_PER_WG - 1 - i];
}

// ---- The sibling rule once more, behind the front seed search: beside a sibling its SHORTCUTS settled ----
// The argument of ScanArgs::min_matches asks nothing of the sibling but its text span [st, en): a missed right piece counts only
// inside [en, n), a missed left piece only inside [0, st) -- an alignment that leaves that region is discordant (lf.end > rf.start,
// span_locater.rs:59-65), one that stays inside has count_matches() <= its text span <= the region -- so with fewer than min_matches
// bases there the read's span is None whatever the missed piece's alignment is, and whether or not the sibling passes the threshold
// itself.  For a sibling settled by a shortcut of flank_window_kernel the span in span4 is the reference's (the proofs there), and the
// front seed search has written it before this kernel starts, on the same stream.  The windowed launch of the other stream writes
// n_match and span4 of OTHER jobs of that list at the same time: nothing is read here but the settled mark, which only the front
// seed search writes, and the span4 entry it stands for.  One thread per job of the list without seeds; the jobs that stay are
// compacted (one atomic per wave) into the pre-filter's list, a dropped job keeps n_match = -1 as after the scan's drop.
//
// ---- ... and the common-subsequence rule, in the same pass ----
// |Adm| is the crudest bound on count_matches() of an alignment inside the admissible region Adm; the sharp one costs about one level
// of the pre-filter.  The matched bases of an alignment of the piece P that stays inside Adm are, in order, a common subsequence of P
// and T[Adm], so count_matches() <= LCS(P, T[Adm]); an alignment that leaves Adm is discordant as before.  With LCS(P, T[Adm]) <
// min_matches the read's span is None whatever the aligner returns -- no tie-breaking, no wavefront enters the argument -- and the job
// is dropped like the others (n_match stays -1).  The sibling's span must be the reference's and must be readable without a race: found
// exactly (pos[sib] >= 0: the scan wrote it, nothing writes it again) or settled by a shortcut (the mark and its span4 entry, as above;
// only where the settled rule is on, a.settled is NULL otherwise).  A byte outside ACGT, in the piece or in the read, counts as
// matching everything, which can only raise the bound.  Pieces of up to LCS_MAX_F bases, regions of min_matches .. lcs_max_adm bases:
// beyond LCS_MAX_ADM the bound hardly ever certifies anything (the census of tools/sibling_census.py) and the
// pass would only be longer.
constexpr int LCS_MAX_F = 256, LCS_MAX_ADM = 352;
struct SettledArgs {
  const JobDev* jobs; const uint32_t* n_jobs;  // the expensive jobs without seeds (count[SC_NOSEED])
  JobDev* out; uint32_t* count;                // the jobs that stay, under count[SC_FILTER]; the others are tallied in count[SC_SETDROP] / count[SC_LCSDROP]
  const uint8_t* settled; const uint32_t* span4; int32_t min_matches;  // (settled NULL: the settled rule is off, and so is everything beside a settled sibling)
  int32_t lcs_max_adm;  // > 0: the common-subsequence rule, over regions of up to this many bases
  const int32_t* pos; const uint8_t* flank_blob; const uint8_t* read_blob;
};
// Is the longest common subsequence of pat[0, F) and txt[0, n) shorter than min_matches?  Bit-parallel (Crochemore et al. 2001, Hyyro
// 2004): one bit per base of the piece in eight dwords, V all ones, per text byte u = V & Peq[c]; V = (V + u) | (V - u), where V - u
// is V & ~u (u is a subset of V: no borrow); the LCS is the number of zero bits among the low F.  The bits from F up are in no mask:
// V & ~u keeps them set whatever carry the sum sends through them, so the zero bits of all 256 are counted.  One thread per job: V in
// registers (the loops over its dwords are unrolled), the five masks -- A, C, T, G and "any other byte", which is every base of the
// piece -- in the thread's own column of LDS (peq[c][w][lane]: conflict-free, and never shared, so no barrier).  The piece comes in 32
// bases per round, the text in sixteen, the next sixteen loaded ahead of the 16 x ~50 instructions over the current ones.  F <= 256;
// nothing is read outside the two ranges.
constexpr int LCS_ROWS = 5;
// the mask row of a byte, without a branch: bits 1-2 of 'A', 'C', 'T', 'G' are 0, 1, 2, 3; any other byte (lower case too) has row 4
__device__ __forceinline__ uint32_t lcs_row(uint32_t c) {
  const uint32_t code = (c >> 1) & 3u;
  return ((0x47544341u >> (8u * code)) & 0xFFu) == c ? code : 4u;
}
__device__ __forceinline__ void lcs_step(uint32_t (&V)[8], const uint32_t (*peq)[8][64], uint32_t lane, uint32_t c) {
  const uint32_t row = lcs_row(c);
  uint32_t m[8], carry = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) m[w] = peq[row][w][lane];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const uint32_t u = V[w] & m[w];
    const uint32_t sum = __builtin_addc(V[w], u, carry, &carry);
    V[w] = sum | (V[w] & ~u);
  }
}
__device__ __forceinline__ bool lcs_below(uint32_t (*peq)[8][64], uint32_t lane, const uint8_t* __restrict__ pat, int F, const uint8_t* __restrict__ txt, int n, int min_matches) {
  for (int w = 0; w < 8; ++w) {  // the masks of bases [32 w, 32 w + 32) of the piece
    uint32_t x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int b0 = w * 32 + q * 4;
      x[q] = 0;
      if (b0 + 4 <= F) x[q] = load_u32(pat + b0);
      else
        for (int k = 0; b0 + k < F; ++k) x[q] |= (uint32_t)pat[b0 + k] << (8 * k);
    }
    uint32_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t row = lcs_row((x[q] >> (8 * k)) & 0xFFu), sel = (1u << row) | (0u - (row >> 2));  // one mask, or all four
        m0 |= (sel & 1u) << (q * 4 + k); m1 |= ((sel >> 1) & 1u) << (q * 4 + k); m2 |= ((sel >> 2) & 1u) << (q * 4 + k); m3 |= ((sel >> 3) & 1u) << (q * 4 + k);
      }
    const uint32_t valid = F >= (w + 1) * 32 ? 0xFFFFFFFFu : (F > w * 32 ? (1u << (F - w * 32)) - 1u : 0u);  // (the zero bytes behind the piece are no bases)
    peq[0][w][lane] = m0 & valid; peq[1][w][lane] = m1 & valid; peq[2][w][lane] = m2 & valid; peq[3][w][lane] = m3 & valid; peq[4][w][lane] = valid;
  }
  uint32_t V[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) V[w] = 0xFFFFFFFFu;
  const int full = n & ~15;
  uint32_t cur[4] = {0, 0, 0, 0}, nxt[4] = {0, 0, 0, 0};
  if (full) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cur[k] = load_u32(txt + 4 * k);
  }
  for (int i = 0; i < full; i += 16) {
    if (i + 16 < full) {
#pragma unroll
      for (int k = 0; k < 4; ++k) nxt[k] = load_u32(txt + i + 16 + 4 * k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int b = 0; b < 4; ++b) lcs_step(V, peq, lane, (cur[k] >> (8 * b)) & 0xFFu);
#pragma unroll
    for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
  }
  for (int i = full; i < n; ++i) lcs_step(V, peq, lane, txt[i]);
  int ones = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) ones += __popc(V[w]);
  return 256 - ones < min_matches;
}
__global__ void __launch_bounds__(64) settled_sibling_kernel(const SettledArgs a) {  // (64: one wave, lcs_below's LDS columns are per lane)
  __shared__ uint32_t l_peq[LCS_ROWS][8][64];
  const uint32_t n = *a.n_jobs, lane = threadIdx.x & 63u;
  for (uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u; i0 < n; i0 += gridDim.x * blockDim.x) {  // (i0: uniform per wave)
    const uint32_t i = i0 + lane;
    bool stay = false, drop = false, lcs = false;
    JobDev jd;
    if (i < n) {
      jd = a.jobs[i];
      const uint32_t j = jd.out_index, sib = j ^ 1u;
      int room = 0x7FFFFFFF, st = 0, en = 0;  // bases of the read on the far side of the sibling (txt_len: the whole read, these jobs have no window)
      bool known = false;
      if (a.settled && a.settled[sib]) {
        st = (int)a.span4[4 * (uint64_t)sib + 2]; en = (int)a.span4[4 * (uint64_t)sib + 3]; known = true;
        room = (j & 1u) ? (int)jd.txt_len - en : st;
        drop = room < a.min_matches;
      } else if (a.lcs_max_adm > 0) {
        st = a.pos[sib]; en = st + (int)jd.pat_len; known = st >= 0;
        if (known) room = (j & 1u) ? (int)jd.txt_len - en : st;
      }
      if (known && !drop && a.lcs_max_adm > 0 && jd.pat_len <= (uint32_t)LCS_MAX_F && room >= a.min_matches && room <= a.lcs_max_adm && (uint32_t)room <= jd.txt_len)
        lcs = lcs_below(l_peq, lane, a.flank_blob + jd.pat_off, (int)jd.pat_len, a.read_blob + jd.txt_off + ((j & 1u) ? (uint32_t)en : 0u), room, a.min_matches);
      stay = !drop && !lcs;
    }
    const unsigned long long ms = __ballot(stay), md = __ballot(drop), ml = __ballot(lcs);
    uint32_t base = 0;
    if (lane == 0) {
      if (ms) base = atomicAdd(a.count + SC_FILTER, (uint32_t)__popcll(ms));
      if (md) atomicAdd(a.count + SC_SETDROP, (uint32_t)__popcll(md));
      if (ml) atomicAdd(a.count + SC_LCSDROP, (uint32_t)__popcll(ml));
    }
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (stay) a.out[base + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull))] = jd;
  }
}

// After the windowed launch: a windowed alignment whose penalty is within the bound of piece_window's argument IS the alignment of
// the whole read, shifted by the window start; any other goes to the back of the job list and is aligned against the whole read.
struct WinCheckArgs {
  const JobDev* win_jobs; const uint32_t* n_win; const int32_t* score; uint32_t* span4; int32_t* n_match; int32_t s0;
  JobDev* wfa_jobs; uint32_t* wfa_count; uint32_t jobs_cap; const uint64_t* read_off; const uint32_t* read_len;
  JobDev* long_rest; uint32_t long_tlen;  // a long read's alignment whose window did not stand: to the long reads' list (NULL: there is none)
};
__global__ void window_check_kernel(const WinCheckArgs a) {
  const uint32_t n = *a.n_win;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    JobDev jd = a.win_jobs[i];
    const uint32_t j = jd.out_index;
    const int32_t sc = a.score[j];  // -penalty, INT32_MIN when the alignment did not complete
    if (sc != INT32_MIN && -sc <= a.s0 && a.n_match[j] > 0) {
      a.span4[4 * (uint64_t)j + 2] += jd.pad; a.span4[4 * (uint64_t)j + 3] += jd.pad;
    } else {
      a.n_match[j] = -1;
      jd.txt_off = a.read_off[j >> 1]; jd.txt_len = a.read_len[j >> 1]; jd.pad = 0;
      if (a.long_rest && jd.txt_len > a.long_tlen) a.long_rest[atomicAdd(a.wfa_count + SC_LNOSEED, 1u)] = jd;
      else a.wfa_jobs[atomicAdd(a.wfa_count + SC_REST, 1u)] = jd;  // (wfa_jobs: the rest list here)
    }
  }
}

// ---- The back-trace of what the pre-filter keeps, confined to a band ----
// The pre-filter hands over more than a verdict: the optimal penalty s* and the diagonal k_end the run ends on (the first one with
// the pattern consumed at level s*).  A wavefront cell (s, k) depends only on cells (s', k') with |k' - k| <= (s - s') / e, and the
// back-trace from (s*, k_end) reads nothing but such cells: everything it touches lies on the diagonals [k_end - s*, k_end + s*],
// text positions [k_end - s*, k_end + s* + plen).  The alignment of the piece against THAT window, started on those diagonals only,
// computes these cells bit for bit; its other cells can only be smaller than in the full run (fewer sources under the max), so it can
// neither end at a lower level nor, at level s*, on a diagonal below k_end.  band_check_kernel compares the penalty anyway and
// sends what differs to the whole-read launch.  A full run spends its time on the ~tlen + 2 s diagonals of every level; the banded
// one on 2 s* + 2 s + 1.
struct BandArgs {
  const JobDev* keep_jobs; const uint32_t* n_keep; JobDev* band_jobs; JobDev* rest_jobs; uint32_t* count; int32_t s_max;
  const int32_t* score; uint32_t* span4; int32_t* n_match; const uint64_t* read_off; const uint32_t* read_len;
  int32_t i_band, i_rest;  // which counters of the block (SC_BAND / SC_HREST, or SC_LBAND / SC_LREST for the long reads)
};
__global__ void heavy_band_kernel(const BandArgs a) {
  const uint32_t n = *a.n_keep;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    JobDev jd = a.keep_jobs[i];
    const uint32_t pad = jd.pad;
    const int s = (int)((pad >> 16) & 0x7FFFu), plen = (int)jd.pat_len, tlen = (int)jd.txt_len, k_end = (int)(pad & 0xFFFFu) - plen;
    const int t0 = max(0, k_end - s), k_hi = min(k_end + s, tlen), t_end = min(tlen, k_end + s + plen);
    if ((pad >> 31) && s <= a.s_max && k_hi >= t0 && t_end > t0) {
      jd.txt_off += (uint64_t)t0; jd.txt_len = (uint32_t)(t_end - t0); jd.pad = (uint32_t)t0;
      jd.ops_off = (uint64_t)(k_hi - t0);  // the free text start of this job (wfa_fast_kernel<64, 3>)
      jd.cigar_off = (uint64_t)s;          // the penalty it must come out with
      a.band_jobs[atomicAdd(a.count + a.i_band, 1u)] = jd;
    } else {
      jd.pad = 0;
      a.rest_jobs[atomicAdd(a.count + a.i_rest, 1u)] = jd;
    }
  }
}
__global__ void band_check_kernel(const BandArgs a) {
  const uint32_t n = a.count[a.i_band];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    JobDev jd = a.band_jobs[i];
    const uint32_t j = jd.out_index;
    const int32_t sc = a.score[j];  // -penalty, INT32_MIN when the alignment did not complete
    if (sc != INT32_MIN && -sc == (int32_t)jd.cigar_off && a.n_match[j] > 0) {
      a.span4[4 * (uint64_t)j + 2] += jd.pad; a.span4[4 * (uint64_t)j + 3] += jd.pad;
    } else {
      a.n_match[j] = -1;
      jd.txt_off = a.read_off[j >> 1]; jd.txt_len = a.read_len[j >> 1]; jd.pad = 0; jd.ops_off = 0; jd.cigar_off = 0;
      a.rest_jobs[atomicAdd(a.count + a.i_rest, 1u)] = jd;
      atomicAdd(a.count + SC_BANDFAIL, 1u);
    }
  }
}

struct CombineArgs {
  uint64_t n_reads; int32_t flank_len; double threshold;
  const int32_t* pos; const int32_t* n_match; const uint32_t* span4;
  int32_t* span_start; int32_t* span_end; uint8_t* lf_hit; uint8_t* rf_hit;
  const uint32_t* count; unsigned long long* cells;  // count[7] (alignments settled by the substitution shortcut) -> cells[2], next to the offset counters
};

__global__ void span_combine_kernel(const CombineArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0 && a.cells) a.cells[2] = a.count[SC_SHORTCUT];
  if (r >= a.n_reads) return;
  int s[2], e[2], hit[2];
  for (int side = 0; side < 2; ++side) {
    const uint64_t j = 2 * r + side;
    s[side] = e[side] = -1; hit[side] = 0;
    if (a.pos[j] >= 0) { s[side] = a.pos[j]; e[side] = a.pos[j] + a.flank_len; hit[side] = 1; }
    else if ((double)(uint64_t)(uint32_t)a.n_match[j] >= a.threshold && a.n_match[j] >= 0) {  // span_locater.rs:18-22
      s[side] = (int)a.span4[4 * j + 2]; e[side] = (int)a.span4[4 * j + 3]; hit[side] = 2;
    }
  }
  int ss = -1, ee = -1;
  if (hit[0] && hit[1] && e[0] <= s[1]) { ss = e[0]; ee = s[1]; }  // :59-65
  a.span_start[r] = ss; a.span_end[r] = ee;
  if (a.lf_hit) a.lf_hit[r] = (uint8_t)hit[0];
  if (a.rf_hit) a.rf_hit[r] = (uint8_t)hit[1];
}

__global__ void cells_merge_kernel(unsigned long long* total2, const unsigned long long* heavy) { total2[1] = heavy[0]; total2[0] += heavy[0]; }

// ---- reads beyond the dedicated kernels' texts (alleles of kilobases): the pre-filter judges them WINDOW BY WINDOW.
// An optimal ends-free alignment of a flank piece costs at most o + plen e (the piece deleted as a whole), so it inserts at most that
// many bases and covers at most span_max = 2 plen + o text bases: with windows of wl bases every `step` = wl - span_max bases (and one
// flush with the end of the read) every alignment the whole read admits lies inside a window, with the same penalty and the same
// matches.  If the filter rejects every window -- no alignment of the window that can still be optimal has min_matches matches -- then
// no alignment of the read has, whichever of the co-optimal ones WFA2-lib would return: the job is dropped as the filter drops a
// short one.  A job with a window that is kept (or could not be judged) goes to the exact kernel with its whole read, as before.
struct LongWinArgs {
  const JobDev* jobs; const uint32_t* n_jobs;  // the long list and its length
  JobDev* sub; uint32_t* parent; uint8_t* sub_keep; uint32_t* n_sub; uint32_t cap;
  uint8_t* job_keep;                           // per long job: 1 = to the exact kernel
  JobDev* kept; uint32_t* n_kept;
  int32_t wl, step;
  // The windows also say WHERE the alignment of a kept job is (FilterArgs::band): every alignment the read admits lies inside a window
  // with the same penalty, so the read's optimal penalty is the smallest one a window reports and its end diagonal the smallest among
  // those windows (a terminating diagonal of a window's run terminates in the whole read's run too, and the first one of the read is
  // the first one of the window that holds its alignment).  That holds when every window either completed or was rejected at a level
  // above that penalty; then the kept job carries penalty and diagonal for the banded back-trace (heavy_band_kernel), else 0.
  const uint32_t* sub_band; uint32_t* job_best; uint32_t* job_rej;  // per long job: min (penalty << 16 | biased end diagonal in the read) | min level of a rejected window (0: a window was not judged)
};
__device__ __forceinline__ uint32_t long_windows_of(uint32_t tlen, int wl, int step) {
  return tlen <= (uint32_t)wl ? 1u : (tlen - (uint32_t)wl + (uint32_t)step - 1u) / (uint32_t)step + 1u;
}
// The windows of a job take a range of the list reserved with one atomic (their order in the list does not matter).  A job whose range
// passes the end of the list is kept unseen; the part of its range that is inside the list is filled with copies of its first window,
// so that the list [0, min(n_sub, cap)) holds valid jobs only.
__global__ void long_windows_kernel(const LongWinArgs a) {
  const uint32_t n = *a.n_jobs;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const JobDev job = a.jobs[j];
    const uint32_t tlen = job.txt_len, nw = long_windows_of(tlen, a.wl, a.step);
    const uint32_t off = atomicAdd(a.n_sub, nw);
    const bool fits = off <= a.cap && nw <= a.cap - off;
    a.job_keep[j] = fits ? 0 : 1;
    if (a.job_best) { a.job_best[j] = 0xFFFFFFFFu; a.job_rej[j] = fits ? 0xFFFFFFFFu : 0u; }
    for (uint32_t w = 0; w < nw && off + w < a.cap; ++w) {
      uint32_t start = fits ? w * (uint32_t)a.step : 0u;
      if (tlen > (uint32_t)a.wl && start + (uint32_t)a.wl > tlen) start = tlen - (uint32_t)a.wl;  // the last window: flush with the end
      JobDev sj = job;
      sj.txt_off = job.txt_off + start; sj.txt_len = tlen > (uint32_t)a.wl ? (uint32_t)a.wl : tlen; sj.out_index = off + w;
      a.sub[off + w] = sj; a.parent[off + w] = j;
    }
  }
}
__global__ void long_verdict_kernel(const LongWinArgs a) {  // a kept window keeps its job
  const uint32_t n = min(*a.n_sub, a.cap);
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const uint32_t p = a.parent[s];
    if (a.sub_keep[s]) a.job_keep[p] = 1;
    if (a.sub_band) {
      const uint32_t b = a.sub_band[s];
      if (b >> 31) {
        const uint64_t kbg = (uint64_t)(b & 0xFFFFu) + (a.sub[s].txt_off - a.jobs[p].txt_off);  // the diagonal counted from the start of the read
        if (kbg < 0x10000u) atomicMin(a.job_best + p, (b & 0x7FFF0000u) | (uint32_t)kbg);
        else atomicMin(a.job_rej + p, 0u);
      } else atomicMin(a.job_rej + p, (b >> 30) ? (b & 0x3FFFFFFFu) : 0u);
    }
  }
}
__global__ void long_kept_kernel(const LongWinArgs a) {
  const uint32_t n = *a.n_jobs;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    if (a.job_keep[j]) {
      JobDev jd = a.jobs[j];
      jd.pad = 0;
      if (a.job_best) {
        const uint32_t best = a.job_best[j];
        if (best != 0xFFFFFFFFu && (best >> 16) < a.job_rej[j]) jd.pad = 0x80000000u | best;
      }
      a.kept[atomicAdd(a.n_kept, 1u)] = jd;
    }
}

// ---- The plan of a find_spans_device call: everything that is decided, once, by span_plan() and before anything is enqueued (no HIP
// call, no buffer of the context).  The stages of SpanCall (below) read the plan and no flank-planning knob.
struct SpanPlan {
  int64_t min_matches = 0; double threshold = 0; int32_t scan_min_matches = 0;  // the smallest count_matches() that passes; the combine's test; the scan's sibling rule (0: off)
  int ring_slots = 0; uint32_t long_tlen = 0, short_max = 0, heavy_tlen_max = 0; bool has_long = false;
  int32_t win_m = WIN_SEGMENTS_DEFAULT, win_q = 0, win_s0 = 0, win_margin = 0, win_spread = 0, win_tbf = 0; uint32_t win_tlen = 0;  // seeded windows (win_q == 0: none)
  int32_t hamming_max = 0, indel_ok = 0; bool win_reg = false;  // (win_reg: the windowed launch is the register kernel's, wfa_win.hip)
  bool split = false, use_filter = false, two_streams = false; int64_t flt_tlen = 0;
  bool heavy_window = false;  // the seed search runs over the expensive list as well
  bool settled_rule = false;  // ... and the sibling rule is applied once more to what that search leaves without seeds (SettledArgs)
  int32_t lcs_max_adm = 0;    // ... as is the common-subsequence rule, over regions of up to this many bases (0: off)
  bool sibling_pass = false;  // either of the two: settled_sibling_kernel compacts the list without seeds into the pre-filter's
  bool heavy_band = false;    // ... and what the pre-filter keeps of it is back-traced inside a band (BandArgs)
  bool band_reg = false;      // ... by the one-wave forward kernel (wfa_band.hip); the LDS launch takes what that leaves
  bool long_window = false;   // the long reads' list goes through the light list's seed search
  bool long_filter = false, long_band = false; int64_t long_wl = 0, long_step = 0; uint64_t long_cap = 0;  // the window filter of the long reads (LongWinArgs)
  int flank_threads = 0, heavy_threads = 0, win_threads = 0, band_threads = 0, band_s_max = 0; bool early_reject = false, count_offsets = false;  // (the last two: of the pre-filter's launches)
};
static SpanPlan span_plan(const trgt_hip_ctx* c, const trgt_span_params& p, uint64_t n_jobs, uint32_t max_read_len, uint32_t heavy_tlen_max, bool have_heavy_len, bool span_only) {
  const trgt_knobs& k = c->knobs;
  const bool wgs = preset_wgs(p.mism, p.gapo, p.gape), filter_pen = preset_has_filter(p.mism, p.gapo, p.gape);
  SpanPlan P;
  // the smallest count_matches() that passes span_locater.rs:18-22
  const double thr = (double)(uint64_t)p.flank_len * p.min_flank_id_frac;
  int64_t min_matches = thr > 0 ? (int64_t)std::ceil(thr) : 0;
  while (min_matches > 0 && (double)(min_matches - 1) >= thr) --min_matches;
  while ((double)min_matches < thr) ++min_matches;
  P.min_matches = min_matches; P.threshold = thr;  // (the combine's test: span_locater.rs:46)
  // (the one-wave-per-piece scan of pieces shorter than four bases does not know the sibling and keeps emitting every job)
  P.scan_min_matches = span_only && !k.no_sibling_rule ? (int32_t)std::min<int64_t>(min_matches, 0x7FFFFFFF) : 0;
  // reads up to long_tlen keep the dedicated kernel at 4 workgroups per CU (LDS: ring + windows <= ~39 KB per alignment)
  P.ring_slots = std::max(p.mism, p.gapo + p.gape) + 1 + 2 * (p.gape + 1);
  const int64_t fit = 39000 / (2 * (int64_t)P.ring_slots + 4) - p.flank_len - 16;
  P.long_tlen = (uint32_t)std::max<int64_t>(fit, 64);
  P.has_long = max_read_len > P.long_tlen;
  P.short_max = P.has_long ? P.long_tlen : max_read_len;
  // Two launches.  The front of the list (reads too short to span their locus: 95 % of the wavefront offsets) holds short texts
  // only, so its launch is planned for heavy_tlen_max: a smaller LDS ring per alignment and one more resident workgroup per CU
  // (occupancy is what this latency-bound kernel lives on: 16.9 -> 15.1 ms from 4 to 5 per CU).  The rest follows at the full size.
  // (a catalog with a few long-read loci has heavy_tlen_max beyond the dedicated kernel's texts: those reads are on the long list
  //  anyway, the launch over the expensive alignments is planned for what is left)
  P.split = have_heavy_len && heavy_tlen_max > 0 && !k.one_launch;
  P.heavy_tlen_max = std::min(heavy_tlen_max, P.short_max);
  // Seeded windows (piece_window): eight segments by default; the conditions make a mismatch the cheapest way to spoil a segment
  // (a gap inside one segment costs o + e, a deletion across t segments o + ((t - 2) q + 2) e >= t x), so that S0 = (segments) x - 1.
  int m = k.win_segments;
  if (m != 4 && m != 6 && m != 8) m = WIN_SEGMENTS_DEFAULT;
  P.win_m = m;
  const int q = p.flank_len / m, x = p.mism, o = p.gapo, e = p.gape;
  if (P.split && !k.no_window && q >= 12 && x >= 1 && e >= 1 && o >= 0 && q * e >= x && o + 2 * e >= 2 * x && o + e >= x) {
    P.win_s0 = x * m - 1;
    const int G = P.win_s0 >= o + e ? (P.win_s0 - o) / e : 0, C = P.win_s0 / e;
    P.win_q = q; P.win_margin = G + C; P.win_spread = 2 * G;
    P.win_tlen = (uint32_t)(p.flank_len + 2 * P.win_margin + P.win_spread);
    if (P.win_tlen + 64 >= max_read_len) P.win_q = 0;  // reads hardly longer than a window
  }
  if (P.win_q > 0) {
    // only the diagonals that can matter start a windowed alignment: a wavefront of 2 margin + spread + 1 diagonals instead of one per
    // base of the window, i.e. one strip of one wave per level
    P.win_tbf = 2 * P.win_margin + P.win_spread;
    P.hamming_max = k.no_hamming ? 0 : std::min(std::min(P.win_m - 1, (p.gapo + p.gape - 1) / p.mism), 4);  // (4: the kernel's count is exact up to there)
    P.indel_ok = !k.no_hamming && !k.no_indel_shortcut && wgs && P.hamming_max == 2 ? 1 : 0;
    // one wave per job with wavefronts and history in registers (wfa_win.hip) where its layout holds the launch; else, and under
    // TRGT_WIN_LDS (developer build: A/B, tests), the LDS kernel.  The register kernel counts no wavefront offsets.
    P.win_reg = !k.win_lds && !k.skip_bt && !k.no_spec && wfa_win_fits(p.mism, p.gapo, p.gape, P.win_tbf, P.win_s0, p.flank_len, P.win_tlen);
  }
  const bool band_ok = k.heavy_band > 0 && wgs && !k.no_spec && !k.skip_bt && !k.wfa_no_stage;  // (the banded launch exists as the LDS kernel of TRGT's configuration only)
  P.band_reg = band_ok && !k.band_lds;  // (TRGT_BAND_LDS, developer build: A/B, tests)
  if (P.split) {
    // The expensive alignments first meet the register-resident pre-filter (wfa_reg.hip): exact penalty and an upper bound on
    // count_matches() without history or back-trace; only those whose bound reaches the threshold (a quarter of the jobs, 5 % of
    // the wavefront offsets on the bench workload) are aligned again by the back-tracing kernel.  span_locater.rs:18-22 does
    // nothing with the others but drop them.
    // (texts beyond the filter's diagonals are kept unseen, job by job: a batch with a few long reads still filters the others)
    P.flt_tlen = flank_filter_max_tlen(p.flank_len);
    P.use_filter = filter_pen && P.flt_tlen >= 2 * (int64_t)p.flank_len &&
                   P.heavy_tlen_max >= (uint32_t)p.flank_len && min_matches <= 254 && !k.no_filter;
    // Two streams: the expensive alignments (pre-filter, then the back-tracing kernel over what it keeps) run on the second stream
    // NEXT TO the other fallback alignments (segment search, windowed launch, whole-read launch) instead of in front of them.  The
    // filter is bound by VALU issue at three waves per SIMD, the light launches by latency and by their job-claim atomics: they
    // fill each other's gaps (measured: see DESIGN.md).  Workspace set 1 for the back-tracing launch of that stream.
    P.two_streams = P.use_filter && !k.one_stream;
    // The expensive list first meets the seed search too.  "Too short to span the locus" says nothing about the flank the read DOES
    // hold: a fifth of these alignments have a penalty below 8 (tools/filter_hist.py) -- the pre-filter let them through after a few
    // levels and the back-tracing kernel aligned them a second time, at the end of this stream's chain.  With seeds they are settled
    // by the substitution shortcut or join the windowed launch of the other stream; the pre-filter sees the jobs WITHOUT seeds only.
    P.heavy_window = P.use_filter && P.two_streams && P.win_q > 0 && !k.no_heavy_window;
    // (on where the scan's rule is on -- callers that hand out hit bytes keep both off -- and a shortcut exists that could settle a sibling)
    P.settled_rule = P.heavy_window && P.scan_min_matches > 0 && P.hamming_max > 0 && !k.no_settled_sibling_rule;
    // (the common-subsequence rule: on where the scan's rule is on; beside a settled sibling only where the settled rule is on too)
    P.lcs_max_adm = P.heavy_window && P.scan_min_matches > 0 && p.flank_len <= LCS_MAX_F && !k.no_lcs_rule ? LCS_MAX_ADM : 0;
    P.sibling_pass = P.settled_rule || P.lcs_max_adm > 0;
    P.heavy_band = P.use_filter && band_ok;
  }
  P.long_window = P.has_long && P.win_q > 0 && !k.no_long_window;  // shortcuts and windows do not care how long the read is
  if (P.has_long) {  // the pre-filter over windows of the long reads (see LongWinArgs): what it rejects never reaches the exact kernel
    const int64_t wl = flank_filter_max_tlen(p.flank_len);
    const int64_t span_max = 2 * (int64_t)p.flank_len + p.gapo + 8, step = wl - span_max;
    // It pays where the exact kernel is the generic one (wavefronts in HBM): texts beyond what the LDS kernel of wfa_launch takes
    // (ring of 11 levels x 2 B + 4 B of windows per diagonal in 96 KB: about 3 500 bases for 250-base pieces).  Reads just above the
    // dedicated launches' length (cfg4: up to 1 300 bases) go to that LDS kernel, and the extra filter launch cost 5 % there.
    const int64_t lds_kernel_tlen = (96 * 1024) / (2 * P.ring_slots + 4) - p.flank_len - 32;
    P.long_filter = filter_pen && min_matches >= 1 && min_matches <= 254 && step >= 256 && (int64_t)max_read_len > lds_kernel_tlen &&
                    !k.no_filter && !k.no_long_filter;
    if (P.long_filter) {
      const uint64_t w_max = (uint64_t)((int64_t)max_read_len > wl ? ((int64_t)max_read_len - wl + step - 1) / step + 1 : 1);
      P.long_cap = std::min<uint64_t>((uint64_t)n_jobs * w_max, 1ull << 21);
      P.long_wl = wl; P.long_step = step;
      P.long_band = band_ok && max_read_len < 0xF000u;
    }
  }
  P.flank_threads = k.flank_threads; P.win_threads = k.win_threads; P.band_threads = k.band_threads; P.band_s_max = k.heavy_band;
  // three waves per expensive alignment: the wavefronts of these short texts are narrow (on average less than one 128-diagonal strip per
  // wave and level), and a wave without a strip still pays the per-level prologue and barrier (7.39 -> 7.21 ms)
  P.heavy_threads = k.heavy_threads > 0 ? k.heavy_threads : (k.flank_threads == 256 ? 192 : k.flank_threads);
  P.early_reject = !k.no_early; P.count_offsets = c->timing;
  return P;
}
struct JobList { const JobDev* jobs; const uint32_t* count; };  // a device-built job list and the word that holds its length
struct OnStream2 {  // inside this scope the context's launches go to its second stream
  trgt_hip_ctx* c;
  explicit OnStream2(trgt_hip_ctx* c_) : c(c_) { std::swap(c->stream, c->stream2); }
  ~OnStream2() { std::swap(c->stream, c->stream2); }
};
// The state of one find_spans_device call: arguments, plan, workspace and the three base launch descriptors.  find_spans_device (below)
// runs the stages in order; what a stage leaves for a later one is a member.  The number of fallback alignments is known only on the
// device: the kernels read it there (n_jobs_dev), the workspace is sized for the upper bound (every job falls back), and nothing here
// waits for the GPU -- trgt_locus_batch enqueues this function chunk after chunk.
struct SpanCall {
  trgt_hip_ctx* const c; const trgt_span_params& p; const int64_t n_reads; const uint64_t n_jobs;
  const uint8_t* d_flank; const uint64_t* d_piece_off; const uint8_t* d_reads; const uint64_t* d_read_off; const uint32_t* d_read_len; const uint32_t* d_read_locus;
  const uint32_t max_read_len; int32_t* d_span_start; int32_t* d_span_end; uint8_t* d_lf_hit; uint8_t* d_rf_hit; const uint32_t* d_heavy_len;
  const SpanPlan plan;
  // workspace (long_noseed: the long reads' list behind the seed search, when that runs over it)
  JobDev *wjobs = nullptr, *wjobs_long = nullptr, *winjobs = nullptr, *restjobs = nullptr, *long_noseed = nullptr;
  uint32_t *count = nullptr, *span4 = nullptr; int32_t *pos = nullptr, *nmatch = nullptr, *score = nullptr;
  uint8_t* settled = nullptr;  // the marks of what the front seed search's shortcuts settled (plan.settled_rule; else NULL)
  // launches: the alignment parameters; the descriptors of the expensive list, the light list (after the seeded windows: the rest list) and the long reads
  trgt_wfa_params wp; WfaLaunch heavy, light, longl;
  JobList long_in{nullptr, nullptr};  // the long reads' list
  bool set_started[2] = {false, false}; void* heavy_cells = nullptr;  // see launch()
  template <class T> int get(int slot, size_t bytes, T*& out) { void* v = nullptr; const int rc = dev_get(c, slot, bytes, &v); out = (T*)v; return rc; }
  int seed_search(bool front, JobDev* rest, JobDev* long_rest);
  int band_backtrace(JobList& list, int slot_band, int slot_rest, int slot_score, int i_band, int i_rest, const WfaLaunch& base, int buffer_set);
  int band_lds_launches(const JobList& kept, JobDev* rest, int slot_band, int slot_score, int i_band, int i_rest, const WfaLaunch& base, int buffer_set);
  // ---- The offset counters (16 bytes per buffer set: [0] a running total, [1] see below).  The first wfa_launch of a call on a buffer
  // set resets that set's counter, every later one keeps counting into it; c->last_wfa_cells_dev, which the caller reads, is the
  // counter of the call's last launch -- one on set 0.  Its [1] holds the offsets of the launches over the expensive list (without
  // two launches: of the one launch over all short reads), the roofline of the dominant launch counts its own: on one stream these
  // are what set 0 has counted when first_launch_done() is called; on two streams they are the total of set 1, merged at the join.
  int launch(const trgt_wfa_params& wpl, WfaLaunch L) {
    bool& started = set_started[L.buffer_set ? 1 : 0];
    L.keep_cells = started; started = true;
    return wfa_launch(c, wpl, L);
  }
  int first_launch_done() {
    if (plan.two_streams) { heavy_cells = c->last_wfa_cells_dev; return TRGT_OK; }
    TRGT_HIP_TRY(c, hipMemcpyAsync((uint8_t*)c->last_wfa_cells_dev + 8, c->last_wfa_cells_dev, 8, hipMemcpyDeviceToDevice, c->stream));
    return TRGT_OK;
  }
  int merge_cells() {  // one counter pair again: [0] all flank alignments, [1] those of the launches over the expensive ones
    hipLaunchKernelGGL(cells_merge_kernel, dim3(1), dim3(1), 0, c->stream, (unsigned long long*)c->last_wfa_cells_dev, (const unsigned long long*)heavy_cells);
    TRGT_HIP_TRY(c, hipGetLastError());
    return TRGT_OK;
  }
  // the stages, in the order find_spans_device calls them
  int workspace(), scan(), heavy_list(), light_windows(), rest_launch(), long_reads(), join_and_combine(), debug_report();
};
int SpanCall::workspace() {  // ... and the base launch descriptors over it
  int rc; void* zeroed = nullptr;
  if ((rc = get(S_FS_POS, n_jobs * 4, pos)) || (rc = get(S_FS_WFAJOBS, n_jobs * sizeof(JobDev), wjobs)) || (rc = dev_get_zeroed(c, S_FS_COUNT, 4 * SC_WORDS, &zeroed, c->stream)) ||
      (rc = get(S_FS_SPAN, n_jobs * 16, span4)) || (rc = get(S_FS_NMATCH, n_jobs * 4, nmatch)))
    return rc;
  count = (uint32_t*)zeroed;
  if (plan.has_long && (rc = get(S_FS_WFAJOBS_LONG, n_jobs * sizeof(JobDev), wjobs_long))) return rc;
  if (plan.settled_rule && (rc = get(S_FS_SETTLED, n_jobs, settled))) return rc;
  if (plan.win_q > 0 && ((rc = get(S_FS_WINJOBS, n_jobs * sizeof(JobDev), winjobs)) || (rc = get(S_FS_RESTJOBS, n_jobs * sizeof(JobDev), restjobs)) ||
                         (rc = get(S_FS_SCORE, n_jobs * 4, score))))
    return rc;
  long_in = {wjobs_long, count + SC_LONG};
  trgt_wfa_default_params(&wp);  // THREAD_WFA_FLANK (genotype.rs:66-80)
  wp.metric = 3; wp.mismatch = p.mism; wp.gap_open1 = p.gapo; wp.gap_ext1 = p.gape;
  wp.span = 1; wp.pattern_begin_free = 0; wp.pattern_end_free = 0; wp.text_begin_free = -1; wp.text_end_free = -1;
  wp.scope = 1; wp.memory_mode = 0; wp.heuristic = 0;
  c->last_wfa_cells_dev = nullptr; c->last_filter_cells_dev = nullptr;
  WfaLaunch L;  // the two-ended list as the scan leaves it, planned for the short reads
  L.jobs_dev = wjobs; L.n_jobs_host = (int64_t)n_jobs; L.n_jobs_dev = count; L.n_jobs2_dev = count + SC_LIGHT; L.jobs_cap = (uint32_t)n_jobs;
  L.pat_base = d_flank; L.txt_base = d_reads;
  L.max_plen = p.flank_len; L.max_tlen = plan.short_max; L.max_sum = (int64_t)p.flank_len + plan.short_max;
  L.threads = plan.flank_threads; L.timer_slot = TRGT_K_WFA_FLANK;
  L.n_match = nmatch; L.span4 = span4;
  heavy = light = longl = L;
  heavy.n_jobs2_dev = nullptr; heavy.jobs_cap = 0;  // the front of the list, on workspace set 1 when it has a stream of its own
  heavy.max_tlen = plan.heavy_tlen_max; heavy.max_sum = (int64_t)p.flank_len + plan.heavy_tlen_max;
  heavy.threads = plan.heavy_threads; heavy.buffer_set = plan.two_streams ? 1 : 0;
  if (plan.split) { light.n_jobs_dev = count + SC_ZERO; light.timer_slot = TRGT_K_WFA_FLANK_REST; }  // (SC_ZERO, always 0: this launch takes the back part of the list only)
  longl.n_jobs2_dev = nullptr; longl.jobs_cap = 0;  // same parameters, workspace and kernel choice planned for the long reads' size
  longl.max_tlen = max_read_len; longl.max_sum = (int64_t)p.flank_len + max_read_len; longl.timer_slot = TRGT_K_WFA_FLANK_REST;
  return TRGT_OK;
}
int SpanCall::scan() {
  ScanArgs sa;
  sa.flank_blob = d_flank; sa.read_blob = d_reads; sa.piece_off = d_piece_off; sa.read_off = d_read_off; sa.read_len = d_read_len;
  sa.read_locus = d_read_locus; sa.n_jobs = n_jobs; sa.flank_len = p.flank_len; sa.pos = pos; sa.n_match = nmatch;
  sa.wfa_jobs = wjobs; sa.wfa_count = count; sa.heavy_len = d_heavy_len; sa.jobs_cap = (uint32_t)n_jobs;
  sa.min_matches = plan.scan_min_matches; sa.settled = settled;
  sa.wfa_jobs_long = wjobs_long; sa.long_tlen = plan.has_long ? plan.long_tlen : 0xFFFFFFFFu;
  KTimer t(c, TRGT_K_FLANK_SCAN);
  if (p.flank_len >= 4) hipLaunchKernelGGL(flank_scan_wide_kernel, dim3((unsigned)((n_reads + SCAN_READS_PER_WG - 1) / SCAN_READS_PER_WG)), dim3(256), 0, c->stream, sa);
  else hipLaunchKernelGGL(flank_scan_kernel, dim3((unsigned)((n_jobs + 3) / 4)), dim3(256), 0, c->stream, sa);
  TRGT_HIP_TRY(c, hipGetLastError());
  t.stop(0);
  tl_mark(c, "scan launched");
  return TRGT_OK;
}
// The seed search on the current stream, over the front of the two-ended list or over its back (then with the long reads' list behind it,
// if long_rest is given): shortcuts, windowed jobs to winjobs, the jobs without a window to rest / long_rest.
int SpanCall::seed_search(bool front, JobDev* rest, JobDev* long_rest) {
  WindowArgs wa;
  wa.flank_blob = d_flank; wa.read_blob = d_reads; wa.wfa_jobs = wjobs; wa.jobs_cap = (uint32_t)n_jobs; wa.count = count;
  wa.win_jobs = winjobs; wa.rest_jobs = rest; wa.flank_len = p.flank_len; wa.q = plan.win_q; wa.margin = plan.win_margin; wa.spread = plan.win_spread; wa.tbf = plan.win_tbf;
  wa.front = front ? 1 : 0; wa.long_jobs = long_rest ? wjobs_long : nullptr; wa.long_rest = long_rest;
  wa.hamming_max = plan.hamming_max; wa.indel_ok = plan.indel_ok;
  wa.n_match = nmatch; wa.span4 = span4; wa.settled = front ? settled : nullptr;  // (the marks are the front search's alone: SettledArgs)
  KTimer t(c, TRGT_K_FLANK_WINDOW);
  const dim3 wgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->num_cus * 8, (int64_t)((n_jobs + WIN_JOBS_PER_WG - 1) / WIN_JOBS_PER_WG))));
  if (plan.win_m == 4) hipLaunchKernelGGL(flank_window_kernel<4>, wgrid, dim3(256), 0, c->stream, wa);
  else if (plan.win_m == 6) hipLaunchKernelGGL(flank_window_kernel<6>, wgrid, dim3(256), 0, c->stream, wa);
  else hipLaunchKernelGGL(flank_window_kernel<8>, wgrid, dim3(256), 0, c->stream, wa);
  TRGT_HIP_TRY(c, hipGetLastError());
  t.stop(0);
  return TRGT_OK;
}
// The banded back-trace (see BandArgs) of a kept list: the alignments inside their band, one wave each, by a launch like `base` on the
// given buffer set; `list` then names whatever is left over for the launch over the whole read.
int SpanCall::band_backtrace(JobList& list, int slot_band, int slot_rest, int slot_score, int i_band, int i_rest, const WfaLaunch& base, int buffer_set) {
  int rc; JobDev* rest = nullptr;
  if ((rc = get(slot_rest, n_jobs * sizeof(JobDev), rest))) return rc;
  const int s_max = plan.band_s_max;
  if (plan.band_reg) {
    // One wave per kept job, forward only (wfa_band.hip): it bands, aligns and checks by itself.  Only a plan that admits penalties or pieces
    // beyond its layout leaves anything on the fallback list; then the three launches below run over that list.
    const bool short_list = i_band == SC_BAND;
    const bool may_fall = s_max > WFA_BAND_S_CAP || p.flank_len > WFA_BAND_PLEN_MAX;
    JobDev* fall = nullptr;
    if (may_fall && (rc = get(short_list ? S_FS_BANDFALL : S_LW_BANDFALL, n_jobs * sizeof(JobDev), fall))) return rc;
    WfaBandLaunch BL;
    BL.jobs_dev = list.jobs; BL.n_jobs_host = (int64_t)n_jobs; BL.n_jobs_dev = list.count; BL.pat_base = d_flank; BL.txt_base = d_reads;
    BL.count = count; BL.i_claim = short_list ? SC_BANDCLAIM : SC_LBANDCLAIM; BL.i_reg = BL.i_claim + 2; BL.i_fall = BL.i_claim + 1;
    BL.i_rest = i_rest; BL.i_fail = SC_BANDFAIL; BL.fall_jobs = fall; BL.rest_jobs = rest;
    BL.n_match = nmatch; BL.span4 = span4; BL.read_off = d_read_off; BL.read_len = d_read_len; BL.s_max = s_max; BL.timer_slot = base.timer_slot;
    if ((rc = wfa_band_launch(c, BL))) return rc;
    list = {rest, count + i_rest};
    if (!may_fall) return TRGT_OK;
    // (the rest list keeps growing: the launch over the whole read comes behind all of this)
    return band_lds_launches(JobList{fall, count + BL.i_fall}, rest, slot_band, slot_score, i_band, i_rest, base, buffer_set);
  }
  if ((rc = band_lds_launches(list, rest, slot_band, slot_score, i_band, i_rest, base, buffer_set))) return rc;
  list = {rest, count + i_rest};
  return TRGT_OK;
}
// ... by the LDS kernel: heavy_band_kernel cuts the windows, wfa_fast_kernel<64, 3> aligns and back-traces, band_check_kernel sorts out
int SpanCall::band_lds_launches(const JobList& kept, JobDev* rest, int slot_band, int slot_score, int i_band, int i_rest, const WfaLaunch& base, int buffer_set) {
  int rc; JobDev* band = nullptr; int32_t* bscore = nullptr;
  if ((rc = get(slot_band, n_jobs * sizeof(JobDev), band)) || (rc = get(slot_score, n_jobs * 4, bscore))) return rc;
  const int s_max = plan.band_s_max;
  BandArgs ba;
  ba.keep_jobs = kept.jobs; ba.n_keep = kept.count; ba.band_jobs = band; ba.rest_jobs = rest; ba.count = count;
  ba.s_max = s_max; ba.score = bscore; ba.span4 = span4; ba.n_match = nmatch;
  ba.read_off = d_read_off; ba.read_len = d_read_len; ba.i_band = i_band; ba.i_rest = i_rest;
  hipLaunchKernelGGL(heavy_band_kernel, dim3(64), dim3(256), 0, c->stream, ba);
  TRGT_HIP_TRY(c, hipGetLastError());
  WfaLaunch LB = base;
  LB.jobs_dev = band; LB.n_jobs_dev = count + i_band;
  LB.max_tlen = (int64_t)p.flank_len + 2 * s_max; LB.max_sum = (int64_t)p.flank_len + LB.max_tlen;
  LB.score = bscore; LB.kernel_tag = 3; LB.max_score = s_max; LB.threads = plan.band_threads; LB.buffer_set = buffer_set;
  trgt_wfa_params wpb = wp;
  wpb.text_begin_free = 2 * s_max;
  if ((rc = launch(wpb, LB))) return rc;
  hipLaunchKernelGGL(band_check_kernel, dim3(64), dim3(256), 0, c->stream, ba);
  TRGT_HIP_TRY(c, hipGetLastError());
  return TRGT_OK;
}
// The expensive list, on the second stream where the plan says so: seed search over the front of the list, the sibling rule beside what
// its shortcuts settled (SettledArgs), pre-filter, banded
// back-trace of what it keeps, back-tracing launch over the rest of that.  Leaves the event the join waits for.
int SpanCall::heavy_list() {
  int rc;
  std::optional<OnStream2> on_stream2;
  if (plan.two_streams) {
    if (!c->stream2) TRGT_HIP_TRY(c, trgt::make_stream(c, &c->stream2));
    if (!c->ev_scan) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&c->ev_scan, hipEventDisableTiming));
    if (!c->ev_heavy) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&c->ev_heavy, hipEventDisableTiming));
    TRGT_HIP_TRY(c, hipEventRecord(c->ev_scan, c->stream));
    TRGT_HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_scan, 0));
    on_stream2.emplace(c);
  }
  JobList list{wjobs, count + SC_HEAVY};
  if (plan.heavy_window) {
    JobDev* noseed = nullptr;
    if ((rc = get(S_FS_NOSEED, n_jobs * sizeof(JobDev), noseed))) return rc;
    if (!c->ev_hwin) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&c->ev_hwin, hipEventDisableTiming));
    if ((rc = seed_search(true, noseed, nullptr))) return rc;
    TRGT_HIP_TRY(c, hipEventRecord(c->ev_hwin, c->stream));
    list = {noseed, count + SC_NOSEED};
    if (plan.sibling_pass) {  // (behind the event: the other stream's seed search does not wait for this)
      JobDev* fjobs = nullptr;
      if ((rc = get(S_FS_FILTERJOBS, n_jobs * sizeof(JobDev), fjobs))) return rc;
      SettledArgs sg;
      sg.jobs = list.jobs; sg.n_jobs = list.count; sg.out = fjobs; sg.count = count;
      sg.settled = settled; sg.span4 = span4; sg.min_matches = plan.scan_min_matches;  // (settled: NULL where the settled rule is off)
      sg.lcs_max_adm = plan.lcs_max_adm; sg.pos = pos; sg.flank_blob = d_flank; sg.read_blob = d_reads;
      // one wave per workgroup: a wave of the common-subsequence rule runs for tens of microseconds and should have a SIMD to itself
      const unsigned sgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->num_cus * 4, (n_jobs + 63) / 64));
      hipLaunchKernelGGL(settled_sibling_kernel, dim3(sgrid), dim3(64), 0, c->stream, sg);
      TRGT_HIP_TRY(c, hipGetLastError());
      list = {fjobs, count + SC_FILTER};
    }
  }
  if (plan.use_filter) {
    JobDev* keepjobs = nullptr;
    if ((rc = get(S_FS_KEEPJOBS, n_jobs * sizeof(JobDev), keepjobs))) return rc;
    FilterLaunch FL;
    FL.jobs_dev = list.jobs; FL.n_jobs_host = (int64_t)n_jobs; FL.n_jobs_dev = list.count;
    FL.pat_base = d_flank; FL.txt_base = d_reads; FL.max_plen = p.flank_len; FL.max_tlen = std::min<int64_t>(plan.heavy_tlen_max, plan.flt_tlen);
    FL.mism = p.mism; FL.gapo = p.gapo; FL.gape = p.gape; FL.count_offsets = plan.count_offsets; FL.min_matches = (int32_t)plan.min_matches; FL.early_reject = plan.early_reject;
    FL.keep_jobs = keepjobs; FL.keep_count = count + SC_KEEP;
    if ((rc = flank_filter_launch(c, FL))) return rc;
    tl_mark(c, "filter launched");
    list = {keepjobs, count + SC_KEEP};
  }
  if (plan.heavy_band && (rc = band_backtrace(list, S_FS_BANDJOBS, S_FS_HRESTJOBS, S_FS_BSCORE, SC_BAND, SC_HREST, heavy, heavy.buffer_set))) return rc;
  WfaLaunch LH = heavy;
  LH.jobs_dev = list.jobs; LH.n_jobs_dev = list.count;
  if ((rc = launch(wp, LH))) return rc;
  tl_mark(c, "heavy launch");
  if ((rc = first_launch_done())) return rc;
  if (plan.two_streams) TRGT_HIP_TRY(c, hipEventRecord(c->ev_heavy, c->stream));
  return TRGT_OK;
}
// The alignments of the light list with a seeded window: short texts, more of them per CU; then sort out which of them stand.
int SpanCall::light_windows() {
  int rc;
  // (the other stream's seed search appends to the same windowed list; this stream's search waits for it rather than running next to
  //  it: the pre-filter behind that one is the critical path of a call, this stream has 0.5 ms of slack -- side by side the short
  //  search took 0.34 instead of 0.08 ms)
  if (plan.heavy_window) TRGT_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_hwin, 0));
  if (plan.long_window) {  // the long reads' alignments meet the seed search too
    if ((rc = get(S_FS_LONGNOSEED, n_jobs * sizeof(JobDev), long_noseed))) return rc;
    long_in = {long_noseed, count + SC_LNOSEED};
  }
  if ((rc = seed_search(false, restjobs, long_noseed))) return rc;
  if (plan.win_reg) {
    WfaWinLaunch WR;
    WR.jobs_dev = winjobs; WR.n_jobs_host = (int64_t)n_jobs; WR.n_jobs_dev = count + SC_WIN; WR.pat_base = d_flank; WR.txt_base = d_reads;
    WR.tbf = plan.win_tbf; WR.s_max = plan.win_s0; WR.counter = count + SC_WINCLAIM; WR.fallback = count + SC_WINFALL;
    WR.score = score; WR.n_match = nmatch; WR.span4 = span4; WR.timer_slot = light.timer_slot;
    if ((rc = wfa_win_launch(c, WR))) return rc;
  } else {
    WfaLaunch LW = light;
    LW.jobs_dev = winjobs; LW.n_jobs_dev = count + SC_WIN; LW.n_jobs2_dev = nullptr; LW.jobs_cap = 0;
    LW.max_tlen = plan.win_tlen; LW.max_sum = (int64_t)p.flank_len + plan.win_tlen;
    LW.score = score; LW.kernel_tag = 2; LW.max_score = plan.win_s0; LW.threads = plan.win_threads;
    trgt_wfa_params wpw = wp;
    wpw.text_begin_free = plan.win_tbf;
    if ((rc = launch(wpw, LW))) return rc;
  }
  tl_mark(c, "window launch");
  WinCheckArgs wc;
  wc.win_jobs = winjobs; wc.n_win = count + SC_WIN; wc.score = score; wc.span4 = span4; wc.n_match = nmatch; wc.s0 = plan.win_s0;
  wc.wfa_jobs = restjobs; wc.wfa_count = count; wc.jobs_cap = (uint32_t)n_jobs;
  wc.read_off = d_read_off; wc.read_len = d_read_len; wc.long_rest = long_noseed; wc.long_tlen = plan.long_tlen;
  hipLaunchKernelGGL(window_check_kernel, dim3(256), dim3(256), 0, c->stream, wc);
  TRGT_HIP_TRY(c, hipGetLastError());
  light.jobs_dev = restjobs; light.n_jobs_dev = count + SC_REST; light.n_jobs2_dev = nullptr; light.jobs_cap = 0;
  return TRGT_OK;
}
int SpanCall::rest_launch() {  // the light list against the whole read -- without two launches: every short read's alignment
  if (const int rc = launch(wp, light)) return rc;
  tl_mark(c, "rest launch");
  return plan.split ? TRGT_OK : first_launch_done();
}
// The long reads: their window filter (see LongWinArgs), the banded back-trace of the kept reads whose windows named penalty and end
// diagonal, as for the short reads (BandArgs), and the exact kernel over what is left.
int SpanCall::long_reads() {
  int rc; const uint64_t cap = plan.long_cap; JobList list = long_in;
  if (plan.long_filter) {
    JobDev *sub = nullptr, *kept = nullptr; uint32_t *parent = nullptr, *sband = nullptr, *jbest = nullptr, *jrej = nullptr; uint8_t *subkeep = nullptr, *jobkeep = nullptr; void* lwc = nullptr;
    if ((rc = get(S_LW_SUB, cap * sizeof(JobDev), sub)) ||
        (rc = get(S_LW_PARENT, cap * 4, parent)) || (rc = get(S_LW_SUBKEEP, cap, subkeep)) ||
        (rc = get(S_LW_JOBKEEP, n_jobs, jobkeep)) || (rc = get(S_LW_KEPT, n_jobs * sizeof(JobDev), kept)) ||
        (rc = dev_get_zeroed(c, S_LW_COUNT, 16, &lwc, c->stream)))
      return rc;
    LongWinArgs lw;
    lw.jobs = list.jobs; lw.n_jobs = list.count;
    lw.sub = sub; lw.parent = parent; lw.sub_keep = subkeep; lw.n_sub = (uint32_t*)lwc; lw.cap = (uint32_t)cap;
    lw.job_keep = jobkeep; lw.kept = kept; lw.n_kept = (uint32_t*)lwc + 1; lw.wl = (int32_t)plan.long_wl; lw.step = (int32_t)plan.long_step;
    if (plan.long_band && ((rc = get(S_LW_SUBBAND, cap * 4, sband)) || (rc = get(S_LW_JOBBEST, n_jobs * 4, jbest)) || (rc = get(S_LW_JOBREJ, n_jobs * 4, jrej)))) return rc;
    lw.sub_band = sband; lw.job_best = jbest; lw.job_rej = jrej;
    const dim3 g((unsigned)c->num_cus * 2), b(256);
    hipLaunchKernelGGL(long_windows_kernel, g, b, 0, c->stream, lw);
    TRGT_HIP_TRY(c, hipGetLastError());
    FilterLaunch FW;
    FW.jobs_dev = sub; FW.n_jobs_host = (int64_t)cap; FW.n_jobs_dev = (const uint32_t*)lwc;
    FW.pat_base = d_flank; FW.txt_base = d_reads; FW.max_plen = p.flank_len; FW.max_tlen = plan.long_wl;
    FW.mism = p.mism; FW.gapo = p.gapo; FW.gape = p.gape; FW.min_matches = (int32_t)plan.min_matches; FW.early_reject = plan.early_reject; FW.keep = subkeep; FW.band = sband; FW.set = 1;
    if ((rc = flank_filter_launch(c, FW))) return rc;
    hipLaunchKernelGGL(long_verdict_kernel, g, b, 0, c->stream, lw);
    hipLaunchKernelGGL(long_kept_kernel, g, b, 0, c->stream, lw);
    TRGT_HIP_TRY(c, hipGetLastError());
    list = {kept, (const uint32_t*)lwc + 1};
    if (plan.long_band && (rc = band_backtrace(list, S_LW_BANDJOBS, S_LW_RESTJOBS, S_LW_BSCORE, SC_LBAND, SC_LREST, longl, 0))) return rc;
  }
  WfaLaunch L2 = longl;
  L2.jobs_dev = list.jobs; L2.n_jobs_dev = list.count;
  return launch(wp, L2);
}
int SpanCall::join_and_combine() {
  if (plan.two_streams) {  // the expensive alignments ran on the second stream: wait for it before the spans are combined
    TRGT_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_heavy, 0));
    if (const int rc = merge_cells()) return rc;
  }
  CombineArgs ca;
  ca.n_reads = (uint64_t)n_reads; ca.flank_len = p.flank_len; ca.threshold = plan.threshold;
  ca.pos = pos; ca.n_match = nmatch; ca.span4 = span4;
  ca.span_start = d_span_start; ca.span_end = d_span_end; ca.lf_hit = d_lf_hit; ca.rf_hit = d_rf_hit;
  ca.count = count; ca.cells = (unsigned long long*)c->last_wfa_cells_dev;
  hipLaunchKernelGGL(span_combine_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, c->stream, ca);
  TRGT_HIP_TRY(c, hipGetLastError());
  return TRGT_OK;
}
int SpanCall::debug_report() {  // (synchronises: developer output only)
  uint32_t h[SC_WORDS];
  TRGT_HIP_TRY(c, trgt::stream_wait(c, c->stream));
  TRGT_HIP_TRY(c, hipMemcpy(h, count, 4 * SC_WORDS, hipMemcpyDeviceToHost));
  const bool win = plan.win_q > 0;
  if (win)
    fprintf(stderr, "[spans] fallback alignments: first launch %u, long reads %u, light %u -> windowed %u, whole read %u (that is %u without seeds + %u windows that did not stand), settled by the shortcuts %u (one-base gaps: %u)\n",
            h[SC_HEAVY], h[SC_LONG], h[SC_LIGHT], h[SC_WIN], h[SC_REST], h[SC_LIGHT] - h[SC_WIN] - h[SC_SHORTCUT], h[SC_REST] - (h[SC_LIGHT] - h[SC_WIN] - h[SC_SHORTCUT]), h[SC_SHORTCUT], h[SC_GAPS]);
  if (!win) fprintf(stderr, "[spans] fallback alignments: first launch %u, long reads %u, light %u (no seeded windows for this configuration)\n", h[SC_HEAVY], h[SC_LONG], h[SC_LIGHT]);
  if (win) fprintf(stderr, "[spans+] windowed launch: %s, %u alignments it did not take\n", plan.win_reg ? "one wave per alignment, history in registers" : "LDS kernel", h[SC_WINFALL]);
  if (win && plan.heavy_window) fprintf(stderr, "[spans+] (the seed search ran over the first launch's list too: %u of its %u alignments had no seeds and met the pre-filter; the counts of the windowed list and of the shortcut include the others)\n", h[SC_NOSEED], h[SC_HEAVY]);
  if (plan.has_long) fprintf(stderr, "[spans+] long reads kept by the window filter: back-traced inside a band %u, over the whole read %u\n", h[SC_LBAND] + h[SC_LBANDREG], h[SC_LREST]);
  fprintf(stderr, "[spans+] sibling rule %s: %u missed pieces without a job (fewer than %d bases beside the exactly found sibling)\n", plan.scan_min_matches > 0 ? "on" : "off", h[SC_SIBDROP], plan.scan_min_matches);
  if (win && plan.heavy_window) fprintf(stderr, "[spans+] settled-sibling rule %s: %u jobs without seeds never met the pre-filter (fewer than %d bases beside a sibling the shortcuts settled)\n", plan.settled_rule ? "on" : "off", h[SC_SETDROP], plan.scan_min_matches);
  if (win && plan.heavy_window) fprintf(stderr, "[spans+] common-subsequence rule %s: %u jobs without seeds never met the pre-filter (no common subsequence of %d bases with the %d to %d bases beside a sibling found exactly or settled by the shortcuts); %u met it\n", plan.lcs_max_adm > 0 ? "on" : "off", h[SC_LCSDROP], plan.scan_min_matches, plan.scan_min_matches, plan.lcs_max_adm, plan.sibling_pass ? h[SC_FILTER] : h[SC_NOSEED]);
  if (plan.heavy_band) fprintf(stderr, "[spans+] kept by the pre-filter: %u -> back-traced inside a band %u (did not stand: %u), over the whole read %u\n", h[SC_KEEP], h[SC_BAND] + h[SC_BANDREG], h[SC_BANDFAIL], h[SC_HREST]);
  if (plan.heavy_band || plan.long_band) fprintf(stderr, "[spans+] banded launch: %s, %u + %u alignments left to the LDS kernel\n", plan.band_reg ? "one wave per alignment, forward only" : "LDS kernel", h[SC_BANDFALL], h[SC_LBANDFALL]);
  return TRGT_OK;
}

// Device-side part shared with trgt_locus_batch: everything already resident, results left on the device.
int find_spans_device(trgt_hip_ctx* c, const trgt_span_params& p, int64_t n_reads, const uint8_t* d_flank, const uint64_t* d_piece_off,
                      const uint8_t* d_reads, const uint64_t* d_read_off, const uint32_t* d_read_len, const uint32_t* d_read_locus,
                      uint32_t max_read_len, int32_t* d_span_start, int32_t* d_span_end, uint8_t* d_lf_hit, uint8_t* d_rf_hit,
                      const uint32_t* d_heavy_len, uint32_t heavy_tlen_max, bool span_only) {
  const uint64_t n_jobs = 2ull * (uint64_t)n_reads;
  SpanCall s{c, p, n_reads, n_jobs, d_flank, d_piece_off, d_reads, d_read_off, d_read_len, d_read_locus, max_read_len, d_span_start, d_span_end, d_lf_hit, d_rf_hit, d_heavy_len,
             span_plan(c, p, n_jobs, max_read_len, heavy_tlen_max, d_heavy_len != nullptr, span_only)};
  int rc;
  if ((rc = s.workspace()) || (rc = s.scan())) return rc;
  if (s.plan.split && (rc = s.heavy_list())) return rc;
  if (s.plan.win_q > 0 && (rc = s.light_windows())) return rc;
  if ((rc = s.rest_launch())) return rc;
  if (s.plan.has_long && (rc = s.long_reads())) return rc;
  if ((rc = s.join_and_combine())) return rc;
  return c->knobs.debug ? s.debug_report() : TRGT_OK;
}

}  // namespace trgt

using namespace trgt;

extern "C" int trgt_find_spans_batch(trgt_hip_ctx* c, const trgt_span_params* p, int64_t n_loci, const uint8_t* flank_blob,
                                     const uint64_t* lf_off, const uint32_t* lf_len, const uint64_t* rf_off,
                                     const uint32_t* rf_len, const uint64_t* locus_read_begin, const uint8_t* read_blob,
                                     const uint64_t* read_off, const uint32_t* read_len, int32_t* span_start,
                                     int32_t* span_end, uint8_t* lf_hit, uint8_t* rf_hit) {
  if (!c) return TRGT_ERR_INVALID;
  if (!p || n_loci < 0 || (n_loci > 0 && (!flank_blob || !lf_off || !lf_len || !rf_off || !rf_len || !locus_read_begin ||
                                          !read_blob || !read_off || !read_len || !span_start || !span_end)))
    return fail(c, TRGT_ERR_INVALID, "trgt_find_spans_batch: null argument");
  if (n_loci == 0) return TRGT_OK;
  if (p->flank_len <= 0) return fail(c, TRGT_ERR_INVALID, "trgt_find_spans_batch: flank_len must be positive");
  TRGT_HIP_TRY(c, hipSetDevice(c->device));
  const int64_t n_reads = (int64_t)locus_read_begin[n_loci];
  if (n_reads == 0) return TRGT_OK;
  if (2 * n_reads > 0xFFFFFFF0ll) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_find_spans_batch: too many reads in one call");
  std::vector<uint64_t> piece_off(2 * (size_t)n_loci);
  std::vector<uint32_t> read_locus((size_t)n_reads), heavy_len((size_t)n_loci);
  uint64_t flank_total = 0, read_total = 0;
  uint32_t max_read_len = 0, heavy_tlen_max = 0;
  for (int64_t l = 0; l < n_loci; ++l) {
    if ((int64_t)lf_len[l] < p->flank_len || (int64_t)rf_len[l] < p->flank_len)
      return fail(c, TRGT_ERR_INVALID, "trgt_find_spans_batch: locus %lld flank shorter than flank_len", (long long)l);
    piece_off[2 * l] = lf_off[l] + lf_len[l] - (uint64_t)p->flank_len;  // lf[lf.len()-F..]  (span_locater.rs:38)
    piece_off[2 * l + 1] = rf_off[l];                                    // rf[..F]           (:39)
    flank_total = std::max<uint64_t>(flank_total, std::max(lf_off[l] + lf_len[l], rf_off[l] + rf_len[l]));
    uint32_t ml = 0;
    for (uint64_t r = locus_read_begin[l]; r < locus_read_begin[l + 1]; ++r) { read_locus[r] = (uint32_t)l; ml = std::max(ml, read_len[r]); }
    heavy_len[(size_t)l] = heavy_read_len(ml, p->flank_len);
    heavy_tlen_max = std::max(heavy_tlen_max, heavy_len[(size_t)l]);
  }
  for (int64_t r = 0; r < n_reads; ++r) {
    read_total = std::max<uint64_t>(read_total, read_off[r] + read_len[r]);
    max_read_len = std::max(max_read_len, read_len[r]);
  }
  int rc;
  const uint8_t *d_flank = nullptr, *d_reads = nullptr;
  const uint64_t *d_piece = nullptr, *d_roff = nullptr;
  const uint32_t *d_rlen = nullptr, *d_rloc = nullptr, *d_heavy = nullptr;
  if ((rc = dev_in(c, S_FS_HEAVY, heavy_len.data(), heavy_len.size(), &d_heavy)) ||
      (rc = dev_in(c, S_FS_FLANK, flank_blob, (size_t)flank_total, &d_flank)) ||
      (rc = dev_in(c, S_FS_READS, read_blob, (size_t)read_total, &d_reads)) ||
      (rc = dev_in(c, S_FS_JOBS, piece_off.data(), piece_off.size(), &d_piece)) ||
      (rc = dev_in(c, S_FS_LIST, read_off, (size_t)n_reads, &d_roff)) ||
      (rc = dev_in(c, S_FS_OUT0, read_len, (size_t)n_reads, &d_rlen)) ||
      (rc = dev_in(c, S_FS_OUT1, read_locus.data(), (size_t)n_reads, &d_rloc)))
    return rc;
  DevOut<int32_t> o_s, o_e; DevOut<uint8_t> o_l, o_r;
  if ((rc = o_s.init(c, S_LOCUS_0, span_start, (size_t)n_reads)) || (rc = o_e.init(c, S_LOCUS_1, span_end, (size_t)n_reads)) ||
      (rc = o_l.init(c, S_FS_HIT0, lf_hit, (size_t)n_reads)) || (rc = o_r.init(c, S_FS_HIT1, rf_hit, (size_t)n_reads)))
    return rc;
  if ((rc = find_spans_device(c, *p, n_reads, d_flank, d_piece, d_reads, d_roff, d_rlen, d_rloc, max_read_len, o_s.dev,
                              o_e.dev, o_l.dev, o_r.dev, d_heavy, heavy_tlen_max > 0 ? heavy_tlen_max - 1 : 0, !lf_hit && !rf_hit)))
    return rc;
  if ((rc = o_s.finish(c)) || (rc = o_e.finish(c)) || (rc = o_l.finish(c)) || (rc = o_r.finish(c))) return rc;
  unsigned long long cells[2] = {0, 0}, fcells[2] = {0, 0};  // total, first launch; pre-filter: offsets, alignments kept
  if (c->last_wfa_cells_dev) { const int d2h_rc = trgt::d2h(c, cells, c->last_wfa_cells_dev, 16, c->stream); if (d2h_rc) return d2h_rc; }
  if (c->last_filter_cells_dev) { const int d2h_rc = trgt::d2h(c, fcells, c->last_filter_cells_dev, 16, c->stream); if (d2h_rc) return d2h_rc; }
  TRGT_HIP_TRY(c, trgt::stream_wait(c, c->stream));
  if (c->timing) {
    c->k_cells[TRGT_K_WFA_FLANK] += (int64_t)cells[1]; c->k_cells[TRGT_K_WFA_FLANK_REST] += (int64_t)(cells[0] - cells[1]);
    c->k_cells[TRGT_K_WFA_FILTER] += (int64_t)fcells[0];
  }
  return TRGT_OK;
}
