// trgt_amd/csrc/locus_gt_deep.hpp -- the deep instantiation of the device-side size genotyper: Genotyper::Size loci with more than
// gt::GT_MAX_READS (256) candidate reads, up to GT_DEEP_MAX_READS, for the contexts that opted in (trgt_hip_set_size_max_reads).  The
// reference's default --max-depth is 250 and its reservoir keeps 3 x max_depth reads, so an ordinary run over deep or targeted data hands
// analyze_tr loci of 257 to 750 reads; without this chain every one of them takes the host path of locus.hip.
//
// Same decisions as locus_gt.hpp (genotype_size.rs:6-64, diploid.rs:5-103, haploid.rs:3-30, consensus.rs:113-154, tr.rs:95-101), restated
// for one WORKGROUP of cld::DW threads per locus of the deep size list instead of one wave:
//   cld::deep_select_kernel / cld::deep_filter_kernel   the kept reads, in global lists (shared with the deep cluster chain)
//   deep_size_genotype_kernel   length histogram, diploid / haploid candidates, collapse, intervals, sequence histogram, picks, split();
//                               a locus with majority support is classified and written out, the others write vote groups, alignment jobs
//                               and a RepairPend into the call's RepairBufs (the repair chain of locus.hip is the same for both depths;
//                               needs, reservation and records are repair_queue.hpp's, the job writer is queue_group_scan below)
//   deep_size_finish_kernel     behind the vote: classification against the repaired alleles, reference allele first, outputs
// The sequential scans of the one-wave kernel (histogram insertion, binary-insertion sort, lane-0 loops) are rank sorts and workgroup
// reductions here.  Ties as in locus_cluster_deep.hpp: every "first / last in index order" of a sequential scan is a lexicographic
// (value, index) reduction.  The f64 penalties are those of locus_gt.hpp: one thread sums one candidate in ascending histogram order.
// Segments are compared where they lie in the read blob; per-read state that no single thread walks stays in the global lists.
//
// The FLANK forms of both kernels (contexts that also opted in to trgt_hip_set_flank_device) run the haplotype-tag branch of
// genotype_flank::genotype for a deep locus whose two sizes are at most 10 apart: flank_route / flank_finish of locus_gt.hpp restated for
// the workgroup, see deep_flank_route.  The SNV forms (contexts that opted in to trgt_hip_set_snv_split_device as well, batches that carry
// mismatch offsets) add the other branch, the split by heterozygous SNVs of the flanks (genotype_flank.rs:78-138, 171-290): snv_route of
// locus_gt.hpp restated for the workgroup, see deep_snv_route.  The search of that branch, up to and including the assignment, is
// deep_snv_search: stated once, and also called by the SNV forms behind the deep cluster chain (locus_cluster_flank_deep.hpp).
#pragma once
#include <cstddef>
#include "locus_cluster_deep.hpp"
#include "locus_gt.hpp"

namespace trgt {
namespace gtd {

constexpr int GT_DEEP_MAX_READS = cld::CL_DEEP_MAX_READS;  // one ceiling: the two selection kernels serve both deep lists
constexpr int MAXR = GT_DEEP_MAX_READS;
using cld::DeepArgs; using cld::DT; using cld::DW; using cld::DWAVES; using cld::Red;
using gt::adiff_u;

// The arguments of the FLANK forms.  A struct of its own, like gt::GtFlankArgs: DeepArgs is the argument of every deep kernel, whose
// register allocation follows its size.
struct DeepFlankArgs {
  DeepArgs d;
  const int16_t* hp_tag;  // per read of the batch: the HP tag (-1 = None)
  uint8_t* flank_done;    // [n_loci] gt::FL_*
};
// The arguments of the SNV forms: what gt::SnvArgs adds to gt::GtFlankArgs, and the route's workspace in HBM.  The per-read masks (32 KB at
// the ceiling) and the staged in-region offsets (64 KB at the cap) do not fit beside the 60 KB of DeepSize, of which only tmp and the part
// of the tag route's overlay behind start are dead when the route runs; so both live in global memory, per read slot of the batch like
// snv_read, and the LDS of the SNV forms is that of the FLANK forms.
struct DeepSnvArgs : DeepFlankArgs {
  const int32_t *start_offset, *end_offset;  // per read of the batch (NULL = 0 for every read, as in flank_split)
  const int32_t* mismatch_offsets; const uint64_t* mismatch_off;  // per read r: its ascending offsets in [mismatch_off[r], mismatch_off[r + 1])
  uint8_t* snv_read;      // per read slot of the batch, by position in the kept list: gt::SR_* of a locus the route split
  double ln_match, ln_mis, ln2;  // ln 0.9, ln(1.0 - 0.9), ln 2 as the host's libm rounds them
  int32_t tag_route;      // 1: tags that split the reads are deep_flank_route's (trgt_hip_set_flank_device is on as well); 0: such a locus is the host's
  uint64_t* prof;         // [2 x read slots of the batch] kept read i of a locus: its observed mask at 2 (r0 + i), its value mask behind it
  int32_t* stage;         // [stage_cap = mismatch_off[reads of the batch]] the in-region offsets of a locus' kept reads, packed from mismatch_off[r0] on (a subset of its lists)
  uint64_t stage_cap;
};
template <bool FLANK, bool SNV = false> using DeepArgsOf = std::conditional_t<SNV, DeepSnvArgs, std::conditional_t<FLANK, DeepFlankArgs, DeepArgs>>;
__device__ __forceinline__ const DeepArgs& deep_of(const DeepArgs& a) { return a; }
__device__ __forceinline__ const DeepArgs& deep_of(const DeepFlankArgs& a) { return a.d; }

// exclusive prefix sum of x over the workgroup in thread order, and the total
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t x, uint32_t& total, Red& r) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = x;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
  if (lane == 63) r.u[wave] = inc;
  __syncthreads();
  uint32_t before = 0; total = 0;
  for (int w = 0; w < DWAVES; ++w) { const uint32_t cw = r.u[w]; before += w < wave ? cw : 0u; total += cw; }
  __syncthreads();
  return before + inc - x;
}
__device__ __forceinline__ uint32_t block_min_u32(uint32_t x, Red& r) {
  for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(x, o); x = t < x ? t : x; }
  if ((threadIdx.x & 63) == 0) r.u[threadIdx.x >> 6] = x;
  __syncthreads();
  uint32_t m = r.u[0];
  for (int w = 1; w < DWAVES; ++w) m = r.u[w] < m ? r.u[w] : m;
  __syncthreads();
  return m;
}
__device__ __forceinline__ uint32_t block_max_u32(uint32_t x, Red& r) { return ~block_min_u32(~x, r); }

// cmp_seg of locus.hip (memcmp over the common prefix, then the shorter one first) by ONE thread, on byte strings anywhere in global memory
__device__ __forceinline__ int cmp_seg_thread(const uint8_t* __restrict__ a, uint32_t na, const uint8_t* __restrict__ b, uint32_t nb) {
  const uint32_t m = na < nb ? na : nb;
  uint32_t i = 0;
  for (; i + 8 <= m; i += 8) {
    uint64_t x, y;
    __builtin_memcpy(&x, a + i, 8); __builtin_memcpy(&y, b + i, 8);
    if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;  // byte order is memory order
  }
  for (; i < m; ++i) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return na < nb ? -1 : (na > nb ? 1 : 0);
}

// ---- classification of the kept reads (genotype_size.rs:42-61), reference allele first (tr.rs:95-101) and the outputs of a locus, by the
// workgroup.  ap / aln / civ / gsz are indexed by allele as genotyped; n_al: alleles the reads are classified against.  The tie-breaker
// starts at 1 and flips at every tie, so the k-th tied read (k from 0) gets k & 1: a prefix count over the kept reads.  false: an allele
// exceeds allele_cap (the host path reports the error), nothing was written.
// BY_TAGS (the haplotype-tag route, genotype_flank.rs:43-76): the classification is the assignment by tag instead -- tag 1 -> group 0, tag 2
// -> group 1, the k-th other read of the kept list (k from 0) -> group k & 1, the same prefix count -- and the alleles arrive smaller one
// first: sw = 1 says that allele 0 is tag group 1's.
// BY_SNV (the SNV route, genotype_flank.rs:114-137): likewise, with the assignment the route left in sr (gt::SR_ASSIGN per kept read).
enum { BY_LEN = 0, BY_TAGS = 1, BY_SNV = 2 };
template <int HOW = BY_LEN>
__device__ __forceinline__ bool deep_size_write(const DeepArgs& a, int64_t l, uint64_t r0, int n, int n_gt, int n_al, const uint8_t* const ap[2],
                                                const uint32_t aln[2], const int32_t civ[4], const uint32_t gsz[2], Red& red,
                                                const int16_t* __restrict__ hp = nullptr, int sw = 0, const uint8_t* __restrict__ sr = nullptr) {
  constexpr bool TAGS = HOW == BY_TAGS;
  const gt::GtArgs& g = a.c.g;
  const int tid = threadIdx.x;
  const uint8_t* ref = g.tr_blob + g.tr_off[l]; const uint32_t refn = g.tr_len[l];
  int flip = 0;  // (wave_equal: every wave compares the whole strings, all reach the same answer)
  if (n_gt != 1 && !gt::wave_equal(ap[0], aln[0], ref, refn) && gt::wave_equal(ap[1], aln[1], ref, refn)) flip = 1;
  // (constant indices throughout, selections instead of indexed loads: the small per-allele arrays stay in registers)
  if (aln[0] > g.allele_cap[l] || (n_gt == 2 && aln[1] > g.allele_cap[l])) return false;
  uint32_t ties = 0, h1 = 0;
  for (int base = 0; base < n; base += DW) {
    const int i = base + tid;
    const bool valid = i < n;
    uint32_t d1 = 0, d2 = 0;
    int tag = 0;
    if constexpr (TAGS) { if (valid) tag = (int)hp[r0 + a.sel_read[r0 + i]]; }
    else if constexpr (HOW == BY_SNV) { if (valid) tag = (int)(sr[r0 + i] & gt::SR_ASSIGN); }
    else if (valid && n_al == 2) { const uint32_t ln = a.sel_len[r0 + i]; d1 = adiff_u(ln, aln[0]); d2 = adiff_u(ln, aln[1]); }
    const bool tie = TAGS ? valid && tag != 1 && tag != 2 : HOW == BY_SNV ? false : valid && n_al == 2 && d1 == d2;
    uint32_t total;
    const uint32_t pos = ties + cld::block_rank(tie, total, red);
    if (valid) {
      int cc;
      if constexpr (TAGS) cc = (tie ? (int)(pos & 1u) : tag - 1) ^ sw;
      else if constexpr (HOW == BY_SNV) cc = tag ^ sw;
      else cc = n_al == 2 ? (d1 < d2 ? 0 : (d1 > d2 ? 1 : (int)(pos & 1u))) : 0;
      h1 += (uint32_t)cc;
      const uint32_t rd = a.sel_read[r0 + i];
      g.classification[r0 + rd] = flip ? 1 - cc : cc;
      g.read_rank[r0 + rd] = i;
    }
    ties += total;
  }
  h1 = cld::block_sum_u32(h1, red);
  const int hap0 = n - (int)h1, hap1 = (int)h1;
#pragma unroll
  for (int oi = 0; oi < 2; ++oi) {
    if (oi >= n_gt) break;
    const bool second = (oi == 1) != (flip != 0);  // the allele written in place oi: order = {1, 0} when flipped
    const uint8_t* src = second ? ap[1] : ap[0]; const uint32_t len = second ? aln[1] : aln[0];
    uint8_t* dst = g.allele_blob + g.allele_off[2 * l + oi];
    for (uint32_t b = tid; b < len; b += DW) dst[b] = src[b];
    if (tid == 0) {
      g.allele_len[2 * l + oi] = len;
      g.ci[4 * l + 2 * oi] = second ? civ[2] : civ[0]; g.ci[4 * l + 2 * oi + 1] = second ? civ[3] : civ[1];
      g.num_spanning[2 * l + oi] = second ? hap1 : hap0;
      if (g.gt_size) g.gt_size[2 * l + oi] = (int32_t)(second ? gsz[1] : gsz[0]);
    }
  }
  if (tid == 0) { g.n_alleles[l] = n_gt; g.n_spanning_reads[l] = (uint32_t)n; g.flipped[l] = (uint8_t)flip; }
  return true;
}

// gt::queue_group for the workgroup of a deep locus: thread t takes items t, t + DW, ...; the place of a member among the jobs of its
// group and the CIGAR words of the members before it are workgroup prefixes, carried across the rounds
template <class IsMember, class SegOf>
__device__ __forceinline__ uint32_t queue_group_scan(gt::RGroup* groups, JobDev* jobs, gt::Reserved& at, gt::Seg bb, uint32_t nm, const gt::GroupNeeds& nd, int n, IsMember is_member, SegOf seg, Red& red) {
  const int tid = threadIdx.x;
  const uint32_t g = at.g0;
  if (tid == 0) gt::put_group(groups, at, bb, nm, nd);
  uint32_t k0 = 0; unsigned long long b0 = 0;
  for (int base = 0; base < n; base += DW) {
    const int i = base + tid;
    const bool in = i < n && is_member(i);
    const gt::Seg s = in ? seg(i) : gt::Seg{0, 0};
    uint32_t tk, tb;
    const uint32_t kk = k0 + cld::block_rank(in, tk, red);
    const unsigned long long before = b0 + block_excl_scan_u32(s.len, tb, red);
    if (in) gt::put_job(jobs, at.j0 + kk, bb, s, at.c0 + (unsigned long long)kk * ((unsigned long long)bb.len + 1) + before);
    k0 += tk; b0 += tb;
  }
  at.c0 += nd.cig; at.j0 += nm; at.o0 += nd.out_need; at.s0 += nd.scr_need; ++at.g0;
  return g;
}

struct DeepSize {
  uint32_t ln[MAXR]; uint64_t off[MAXR];  // kept reads in LocusResult.reads order: span length, blob offset of the repeat segment
  uint32_t ulen[MAXR], ucnt[MAXR];        // unique lengths ascending, multiplicities
  uint32_t tmp[MAXR];                     // the sorted lengths; later per kept read: multiplicity of its sequence, bit 31 = an earlier read has it too
  uint16_t ord[MAXR];                     // first read of every length in the sorted list; later the kept reads in byte-lexicographic order (stable)
  uint16_t u_rep[MAXR], u_cnt[MAXR];      // unique sequences in that order: representative (the earliest read), multiplicity
  Red red;
  gt::Reserved rsv;
};
static_assert(sizeof(DeepSize) <= 64 * 1024, "static LDS of the deep size genotyper");

// ---- the haplotype-tag branch of genotype_flank::genotype (genotype_flank.rs:9-76, 147-170; applied at tr.rs:69-75) for a workgroup:
// flank_route / flank_finish of locus_gt.hpp with every lane-0 loop and wave ballot as a workgroup prefix or a (value, index) reduction.
// Its LDS lies over DeepSize::ulen / ucnt, which are dead once the intervals are computed.
struct DeepFlank {
  uint16_t start[MAXR];   // per unique sequence: where its run of equal segments begins in DeepSize::ord
  uint16_t cnt[2][MAXR];  // multiplicity of every unique sequence inside either tag group
  uint8_t grp[MAXR];      // per kept read: its tag group
  uint32_t med[2][2];     // the two middle lengths of either group
};
static_assert(sizeof(DeepFlank) <= 2 * sizeof(uint32_t) * MAXR && offsetof(DeepSize, ucnt) == offsetof(DeepSize, ulen) + sizeof(uint32_t) * MAXR &&
              offsetof(DeepSize, ulen) % alignof(DeepFlank) == 0, "the tag route's LDS lies over ulen / ucnt");
__device__ __forceinline__ DeepFlank& deep_flank_lds(DeepSize& sh) { return *reinterpret_cast<DeepFlank*>(static_cast<void*>(sh.ulen)); }

// get_trs_with_hp (:43-76) over the kept reads in kept order: tag 1 -> group 0, tag 2 -> group 1, the k-th other read (k from 0, a running
// count over the whole list: a workgroup prefix carried across the rounds) -> group k & 1.  true: the split is accepted (both groups
// occur, at least 70 % of the reads tagged).  Uniform arguments, uniform result; grp is visible to every thread on return.
__device__ __forceinline__ bool deep_flank_assign(uint8_t* grp, const DeepArgs& a, const int16_t* __restrict__ hp, uint64_t r0, int n, int cnt[2], Red& red) {
  const int tid = threadIdx.x;
  uint32_t untagged = 0, ones = 0;
  for (int base = 0; base < n; base += DW) {
    const int i = base + tid;
    const bool valid = i < n;
    const int tag = valid ? (int)hp[r0 + a.sel_read[r0 + i]] : 1;
    const bool un = valid && tag != 1 && tag != 2;
    uint32_t total;
    const uint32_t k = untagged + cld::block_rank(un, total, red);
    if (valid) { const uint32_t g = un ? (k & 1u) : (uint32_t)(tag - 1); grp[i] = (uint8_t)g; ones += g; }
    untagged += total;
  }
  ones = cld::block_sum_u32(ones, red);
  cnt[1] = (int)ones; cnt[0] = n - (int)ones;
  return cnt[0] > 0 && cnt[1] > 0 && (double)(n - (int)untagged) / (double)n >= 0.7;
}

// Who belongs to group t of a split, from the byte of a kept read in DeepFlank::grp.  By tags: the byte is the group.  By SNVs (:114-137):
// bit 0 is the assignment, bit 1 says that the read agrees equally with both haplotypes and is a member of both groups.
struct DeepTagMembers { static constexpr bool BOTH = false; static __device__ __forceinline__ bool in(uint32_t b, int t) { return b == (uint32_t)t; } };
struct DeepSnvMembers { static constexpr bool BOTH = true; static __device__ __forceinline__ bool in(uint32_t b, int t) { return (b & 1u) == (uint32_t)t || (b & 2u); } };

// What follows an accepted split (genotype_flank.rs:20-41), behind the sequence histogram (ord, tmp, u_rep, u_cnt, nu final; fl.start
// filled) and the assignment (fl.grp; cnt: the members of either group, MEM says who): simple_consensus (:147-170) of either group;
// without a group below 50 % the genotype is written out, else the groups join the call's repair chain (need_host = 2, the FLANK / SNV
// finish kernel completes the locus) or the locus is handed to the host path (need_host = 1, FL_HANDED).  sr (BOTH only): the SNV
// route's per-read bytes, which hold the assignment.  false (BOTH only): a group is empty, there is no split, nothing was written.
template <class MEM>
__device__ __forceinline__ bool deep_flank_tail(DeepSize& sh, const DeepFlankArgs& fa, int64_t l, uint64_t r0, int n, int nu, const int cnt[2], const uint8_t* __restrict__ sr = nullptr) {
  const DeepArgs& a = fa.d;
  const gt::GtArgs& g = a.c.g;
  DeepFlank& fl = deep_flank_lds(sh);
  const int tid = threadIdx.x;
  constexpr int NONE = 0x7FFFFFFF;
  constexpr uint8_t mark = MEM::BOTH ? (uint8_t)gt::FL_SNV : (uint8_t)0;
  if constexpr (MEM::BOTH) { if (cnt[0] == 0 || cnt[1] == 0) return false; }
  // ---- multiplicities inside the groups (thread q walks the run of unique sequence q), the middle lengths of either group by rank
  for (int q = tid; q < nu; q += DW) {
    const int s = fl.start[q], m = sh.u_cnt[q];
    if constexpr (MEM::BOTH) {
      int c0 = 0, c1 = 0;
      for (int r = s; r < s + m; ++r) { const uint32_t b = fl.grp[sh.ord[r]]; c0 += MEM::in(b, 0); c1 += MEM::in(b, 1); }
      fl.cnt[0][q] = (uint16_t)c0; fl.cnt[1][q] = (uint16_t)c1;
    } else {
      int c1 = 0;
      for (int r = s; r < s + m; ++r) c1 += fl.grp[sh.ord[r]];
      fl.cnt[0][q] = (uint16_t)(m - c1); fl.cnt[1][q] = (uint16_t)c1;
    }
  }
  for (int i = tid; i < n; i += DW) {
    const uint32_t gi = fl.grp[i], li = sh.ln[i];
    if constexpr (MEM::BOTH) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {  // a read of both groups has a rank in either
        if (!MEM::in(gi, t)) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) { const uint32_t lj = sh.ln[j]; r += MEM::in(fl.grp[j], t) && (lj < li || (lj == li && j < i)); }
        const int half = cnt[t] / 2;
        if (r == half) fl.med[t][1] = li;
        if (r == half - 1) fl.med[t][0] = li;
      }
    } else {
      int r = 0;
      for (int j = 0; j < n; ++j) { const uint32_t lj = sh.ln[j]; r += fl.grp[j] == gi && (lj < li || (lj == li && j < i)); }
      const int half = (gi ? cnt[1] : cnt[0]) / 2;
      if (r == half) fl.med[gi][1] = li;
      if (r == half - 1) fl.med[gi][0] = li;
    }
  }
  __syncthreads();
  int rep[2] = {0, 0}; uint32_t aln[2] = {0, 0}, lo[2] = {0, 0}, hi[2] = {0, 0}; bool lacks[2] = {false, false};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    // utils::math::median (math.rs:73-98) as f32, truncated: the middle value, or (a + b) as i32, then / 2.0
    const float med = (cnt[t] & 1) ? (float)(int32_t)fl.med[t][1] : (float)((int32_t)fl.med[t][0] + (int32_t)fl.med[t][1]) / 2.0f;
    const uint32_t median_len = (uint32_t)med;
    uint32_t top = 0;
    for (int q = tid; q < nu; q += DW) top = fl.cnt[t][q] > top ? fl.cnt[t][q] : top;
    top = block_max_u32(top, sh.red);
    // among the sequences with the largest multiplicity, in u_rep order: the first minimum of |len - median|
    double bd = __builtin_huge_val(); int bq = NONE;
    for (int q = tid; q < nu; q += DW)
      if (fl.cnt[t][q] == top) { const double d = (double)adiff_u(sh.ln[sh.u_rep[q]], median_len); if (d < bd) { bd = d; bq = q; } }
    cld::block_min_vi(bd, bq, sh.red);
    uint32_t mn = 0xFFFFFFFFu, mx = 0;
    for (int i = tid; i < n; i += DW) if (MEM::in(fl.grp[i], t)) { const uint32_t li = sh.ln[i]; mn = li < mn ? li : mn; mx = li > mx ? li : mx; }
    lo[t] = block_min_u32(mn, sh.red); hi[t] = block_max_u32(mx, sh.red);
    rep[t] = sh.u_rep[bq == NONE ? 0 : bq]; aln[t] = sh.ln[rep[t]];  // (the group is not empty: some thread has a value)
    lacks[t] = (double)top / (double)cnt[t] < 0.5;
  }
  if (lacks[0] || lacks[1]) {
    // ---- a group below 50 %: backbone = its sequence, one member per read of the group in kept order, duplicates included
    const gt::RepairBufs& rp = g.rp;
    bool can = rp.counts != nullptr;
    uint32_t nm[2] = {0, 0}, mbytes[2] = {0, 0};
    if (can) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (!lacks[t]) continue;
        uint32_t bytes = 0, over = aln[t] > rp.max_seg;
        for (int i = tid; i < n; i += DW) if (MEM::in(fl.grp[i], t)) { const uint32_t li = sh.ln[i]; over += li > rp.max_seg; bytes += li > rp.max_seg ? 0u : li; }
        nm[t] = (uint32_t)cnt[t]; mbytes[t] = cld::block_sum_u32(bytes, sh.red);
        if (cld::block_sum_u32(over, sh.red)) can = false;
      }
    }
    gt::GroupNeeds nd[2] = {};
    if (can) {
#pragma unroll
      for (int t = 0; t < 2; ++t) if (lacks[t]) nd[t] = gt::group_needs(aln[t], nm[t], mbytes[t], rp.vote_lds_pos);
      if (tid == 0) gt::repair_reserve(rp, l, g.n_loci, nm[0] + nm[1], (uint32_t)lacks[0] + (uint32_t)lacks[1], nd, sh.rsv);
      __syncthreads();
      can = sh.rsv.ok != 0;
    }
    if (!can) { if (tid == 0) { g.need_host[l] = 1; fa.flank_done[l] = gt::FL_HANDED | mark; } return true; }
    gt::Reserved at = sh.rsv;
    auto seg_of = [&](int i) { return gt::Seg{sh.off[i], sh.ln[i]}; };
    gt::RepairPend pd;
    pd.n_gt = 2; pd.n_pick = 2 | gt::RP_FLANK | (MEM::BOTH ? gt::RP_SNV : 0); pd.size[0] = aln[0]; pd.size[1] = aln[1];
#pragma unroll
    for (int t = 0; t < 2; ++t) { pd.civ[2 * t] = (int32_t)lo[t]; pd.civ[2 * t + 1] = (int32_t)hi[t]; pd.rep[t] = rep[t]; pd.grp[t] = -1; }
#pragma unroll
    for (int t = 0; t < 2; ++t)  // job k of a group is its k-th read in kept order
      if (lacks[t]) pd.grp[t] = (int32_t)queue_group_scan(rp.groups, rp.jobs, at, seg_of(rep[t]), nm[t], nd[t], n, [&, t](int i) { return MEM::in(fl.grp[i], t); }, seg_of, sh.red);
    if (tid == 0) { rp.pend[l] = pd; g.need_host[l] = 2; }  // the locus waits for the FLANK / SNV form of deep_size_finish_kernel
    return true;
  }
  // ---- both groups have their sequence: smaller allele first (:33-38: alleles and intervals swap, the assignment flips), the
  //      assignment is the classification, then reference allele first (tr.rs:95-101): deep_size_write<BY_TAGS / BY_SNV>
  const int sw = aln[0] > aln[1] ? 1 : 0;
  const uint8_t* ap[2] = {g.reads + sh.off[sw ? rep[1] : rep[0]], g.reads + sh.off[sw ? rep[0] : rep[1]]};
  const uint32_t al2[2] = {sw ? aln[1] : aln[0], sw ? aln[0] : aln[1]};
  const int32_t civ[4] = {(int32_t)(sw ? lo[1] : lo[0]), (int32_t)(sw ? hi[1] : hi[0]), (int32_t)(sw ? lo[0] : lo[1]), (int32_t)(sw ? hi[0] : hi[1])};
  const bool ok = deep_size_write<MEM::BOTH ? BY_SNV : BY_TAGS>(a, l, r0, n, 2, 2, ap, al2, civ, al2, sh.red, fa.hp_tag, sw, sr);
  if (tid == 0) { g.need_host[l] = ok ? 0 : 1; fa.flank_done[l] = (uint8_t)((ok ? gt::FL_DONE : gt::FL_HANDED) | mark); }  // (an allele beyond allele_cap: the host path reports the error)
  return true;
}

// The tag route inside the genotype kernel.  false: the tags do not split the reads and the locus continues with the length genotype.
// true: the locus is settled by deep_flank_tail.
__device__ __forceinline__ bool deep_flank_route(DeepSize& sh, const DeepFlankArgs& fa, int64_t l, uint64_t r0, int n, int nu) {
  int cnt[2];
  if (!deep_flank_assign(deep_flank_lds(sh).grp, fa.d, fa.hp_tag, r0, n, cnt, sh.red)) return false;
  return deep_flank_tail<DeepTagMembers>(sh, fa, l, r0, n, nu, cnt);
}

// ---- the SNV branch of genotype_flank::genotype (get_trs_with_clustering, genotype_flank.rs:78-138, with get_analysis_region, call_snvs,
// the profiles, the candidate genotypes and their log-likelihoods, :171-290) for a workgroup, tried where the tags do not split the reads:
// gt::snv_route with every lane-0 loop and wave ballot as a workgroup prefix, and every selection as a (value, index) rank.  What the
// route decides, when it decides (the margin rule) and why that is safe are snv_route's, see there; the bound on the difference between
// the host's and the device's sum of one candidate grows with the reads of a locus, and for n <= 2 048 its three terms give
// n * 2^-49 + 2^-51 * (|M| + 1.4 n) + n * 2^-52 * |M| < 5e-12 * (1 + |M|), of which the margin 2^-30 * (1 + |M|) is still about 180 times.
// In the deep size kernels the small lists of the search lie over DeepFlank::cnt, which the tail fills only after them, and the offsets
// whose rank is taken over DeepSize::tmp (deep_snv_route, below the search); masks and staged offsets in DeepSnvArgs::prof / stage.
// The limits are shared by both callers: gt::SNV_MAX_SNVS, gt::SNV_MAX_HAPS, SNV_DEEP_CAP.
// false: no split (FL_NOSPLIT | FL_SNV: neither branch splits the reads, the host need not look) and the locus continues with the length
// genotype.  true: settled by deep_flank_tail, or handed to the host path (need_host = 1, FL_HANDED | FL_SNV).
struct DeepSnv {
  uint64_t v_hap[gt::SNV_MAX_HAPS], v_htmp[gt::SNV_MAX_HAPS];  // the distinct fully observed profiles in the derived order of Option<bool> (v_htmp: as found)
  double v_ll[gt::SNV_MAX_HAPS * (gt::SNV_MAX_HAPS + 1) / 2];
  int32_t v_snv[gt::SNV_MAX_SNVS], v_tmp[gt::SNV_MAX_SNVS];    // the called SNVs ascending (v_tmp: as found)
  int32_t v_reg[2];
};
static_assert(sizeof(DeepSnv) <= sizeof(DeepFlank::cnt) && offsetof(DeepFlank, cnt) % alignof(DeepSnv) == 0, "the SNV route's lists lie over the tag route's multiplicities");
constexpr int SNV_DEEP_CAP = gt::SNV_OFFS_PER_READ * MAXR;  // in-region occurrences of a locus: 8 per read slot of the kernel
static_assert(SNV_DEEP_CAP / DW <= 64, "one bit per owned entry in `called`");

// The search itself, up to and including the assignment, stated once for both deep lists (the size route below and the SNV forms of
// locus_cluster_flank_deep.hpp).  sv / key: where its small lists and the offsets whose rank is taken live in LDS (key: n words); grp: per
// kept read, bit 0 the assignment, bit 1 set for a read of both groups; read_of(i): the read of the batch that kept read i is; sa: the
// route's arguments (the fields DeepSnvArgs adds to DeepFlankArgs, under these names); end: how it ends, like clf::ClusterEnd --
//   end.nosplit()     no split          end.handed(why)   beyond a limit (why = 0) or undecided (FL_UNDECIDED)
//   end.split(cnt)    the assignment is in grp and in sa.snv_read (SR_*), cnt[t] members of either group (a group may be empty)
// and the result is what they return.  Every thread is done with sv and key when end.split is called.  Uniform arguments and result.
template <class A, class ReadOf, class End>
__device__ __forceinline__ bool deep_snv_search(DeepSnv& sv, int32_t* const key, uint8_t* const grp, Red& red, const A& sa, uint64_t r0, int n, ReadOf read_of, End& end) {
  const int tid = threadIdx.x;
  auto nosplit = [&]() { return end.nosplit(); };
  auto handed = [&](uint8_t why) { return end.handed(why); };
  // ---- get_analysis_region (:206-226): the skip-th largest start offset, the skip-th smallest end offset, by (value, index) rank
  const int skip = (int)round((double)n * (1.0 - 0.85));
  if (skip >= n) return nosplit();
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int32_t* __restrict__ src = side ? sa.end_offset : sa.start_offset;
    const int want = side ? skip : n - 1 - skip;
    for (int i = tid; i < n; i += DW) key[i] = src ? src[read_of(i)] : 0;
    __syncthreads();
    for (int i = tid; i < n; i += DW) {
      const int32_t v = key[i];
      int r = 0;
      for (int j = 0; j < n; ++j) { const int32_t vj = key[j]; r += vj < v || (vj == v && j < i); }
      if (r == want) sv.v_reg[side] = v;
    }
    __syncthreads();
  }
  const int32_t reg0 = sv.v_reg[0], reg1 = sv.v_reg[1];
  // ---- call_snvs (:271-286): the in-region offsets of all kept reads, packed in kept order (thread i counts and writes the ones of read
  //      i; its place is a workgroup prefix carried across the rounds)
  //      (room: the locus' own part of the table holds them all; a table that does not ascend cannot make a thread write beyond the buffer)
  const uint64_t stage0 = sa.mismatch_off[r0];
  const uint64_t room = stage0 < sa.stage_cap ? sa.stage_cap - stage0 : 0;
  int32_t* const stage = sa.stage + (room ? stage0 : 0);
  uint32_t total = 0;
  for (int base = 0; base < n; base += DW) {
    const int i = base + tid;
    uint64_t m0 = 0, m1 = 0;
    if (i < n) { const uint64_t r = read_of(i); m0 = sa.mismatch_off[r]; m1 = sa.mismatch_off[r + 1]; }
    uint32_t c = 0;
    for (uint64_t k = m0; k < m1; ++k) { const int32_t o = sa.mismatch_offsets[k]; c += reg0 <= o && o <= reg1; }
    uint32_t tot;
    uint32_t at = total + block_excl_scan_u32(c, tot, red);
    for (uint64_t k = m0; k < m1; ++k) { const int32_t o = sa.mismatch_offsets[k]; if (reg0 <= o && o <= reg1) { if (at < room) stage[at] = o; ++at; } }
    total += tot;
  }
  __syncthreads();
  if (total == 0) return nosplit();  // no SNV: every profile is empty, one candidate genotype
  if (total > (uint32_t)SNV_DEEP_CAP || total > room) return handed(0);
  // an offset is called when its occurrences are at least 20 % of the reads; thread e owns entries e, e + DW, ...: the first occurrence speaks
  uint64_t called = 0;  // bit t: entry tid + DW t is the first occurrence of a called offset
  for (int t = 0; t < SNV_DEEP_CAP / DW; ++t) {
    const uint32_t e = (uint32_t)tid + (uint32_t)DW * (uint32_t)t;
    if (e >= total) break;
    const int32_t o = stage[e];
    int c = 0; bool first = true;
    for (uint32_t j = 0; j < total; ++j) { const bool same = stage[j] == o; c += same; first = first && !(same && j < e); }
    if (first && (double)c / (double)n >= 0.20) called |= 1ull << t;
  }
  int ns = 0;
  for (int t = 0; t < SNV_DEEP_CAP / DW; ++t) {
    if ((uint32_t)DW * (uint32_t)t >= total) break;
    const bool mine = (called >> t) & 1ull;
    uint32_t tot;
    const uint32_t at = (uint32_t)ns + cld::block_rank(mine, tot, red);
    if (mine && at < (uint32_t)gt::SNV_MAX_SNVS) sv.v_tmp[at] = stage[(uint32_t)tid + (uint32_t)DW * (uint32_t)t];
    ns += (int)tot;
  }
  __syncthreads();
  if (ns == 0) return nosplit();
  if (ns > gt::SNV_MAX_SNVS) return handed(0);
  if (tid < ns) {  // ascending
    const int32_t o = sv.v_tmp[tid];
    int r = 0;
    for (int j = 0; j < ns; ++j) r += sv.v_tmp[j] < o;
    sv.v_snv[r] = o;
  }
  __syncthreads();
  // ---- profiles (:250-269): SNV k of a read is None outside [start_offset, end_offset], else whether its list has the offset
  const uint64_t all = ns == 64 ? ~0ull : (1ull << ns) - 1ull;
  uint64_t* const prof = sa.prof + 2 * r0;
  uint32_t full = 0;
  for (int i = tid; i < n; i += DW) {
    const uint64_t r = read_of(i);
    const int32_t* m = sa.mismatch_offsets + sa.mismatch_off[r];
    const int nm = (int)(sa.mismatch_off[r + 1] - sa.mismatch_off[r]);
    const int32_t s = sa.start_offset ? sa.start_offset[r] : 0, e = sa.end_offset ? sa.end_offset[r] : 0;
    uint64_t obs = 0, val = 0;
    for (int k = 0; k < ns; ++k) {
      const int32_t o = sv.v_snv[k];
      if (o < s || o > e) continue;
      obs |= 1ull << k;
      int lo = 0, hi = nm;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (m[mid] < o) lo = mid + 1; else hi = mid; }
      if (lo < nm && m[lo] == o) val |= 1ull << k;
    }
    prof[2 * i] = obs; prof[2 * i + 1] = val;
    full += obs == all;
  }
  full = cld::block_sum_u32(full, red);  // (its barriers also publish the masks to the workgroup)
  // ---- candidate genotypes (:228-248): the distinct fully observed profiles in the derived order of Option<bool> -- first SNV most
  //      significant, false before true: the bit-reversed value mask -- and their pairs a <= b, a outer
  if ((double)full / (double)n < 0.40) return nosplit();
  int nh = 0;
  for (int base = 0; base < n; base += DW) {
    const int i = base + tid;
    bool first = i < n && prof[2 * i] == all;
    uint64_t v = 0;
    if (first) { v = prof[2 * i + 1]; for (int j = 0; j < i; ++j) first = first && !(prof[2 * j] == all && prof[2 * j + 1] == v); }
    uint32_t tot;
    const uint32_t q = (uint32_t)nh + cld::block_rank(first, tot, red);
    if (first && q < (uint32_t)gt::SNV_MAX_HAPS) sv.v_htmp[q] = v;
    nh += (int)tot;
  }
  __syncthreads();
  if (nh * (nh + 1) / 2 <= 1) return nosplit();
  if (nh > gt::SNV_MAX_HAPS) return handed(0);
  if (tid < nh) {
    const uint64_t v = sv.v_htmp[tid], kv = __brevll(v);
    int r = 0;
    for (int j = 0; j < nh; ++j) r += __brevll(sv.v_htmp[j]) < kv;
    sv.v_hap[r] = v;
  }
  __syncthreads();
  // ---- log-likelihoods (:171-204), one thread per candidate (at most 136), the reads in kept order: gt::snv_candidate_ll
  const int nc = nh * (nh + 1) / 2;
  for (int c = tid; c < nc; c += DW) {
    int ha = 0, hb = 0;
    { int p = 0; for (int x = 0; x < nh; ++x) for (int y = x; y < nh; ++y, ++p) if (p == c) { ha = x; hb = y; } }
    sv.v_ll[c] = gt::snv_candidate_ll(sa, n, ns, sv.v_hap[ha], sv.v_hap[hb], [&](int i, uint64_t& obs, uint64_t& val) { obs = prof[2 * i]; val = prof[2 * i + 1]; });
  }
  __syncthreads();
  // ---- the decision: max_by's winner is the last maximum in candidate order; every other candidate must stay below M - delta
  double M = sv.v_ll[0]; int win = 0;
  for (int c = 1; c < nc; ++c) if (sv.v_ll[c] >= M) { M = sv.v_ll[c]; win = c; }
  const double delta = 0x1p-30 * (1.0 + fabs(M));
  bool decided = true;
  for (int c = 0; c < nc; ++c) if (c != win && sv.v_ll[c] >= M - delta) decided = false;
  if (!decided) return handed(gt::FL_UNDECIDED);
  int wa = 0, wb = 0;
  { int p = 0; for (int x = 0; x < nh; ++x) for (int y = x; y < nh; ++y, ++p) if (p == win) { wa = x; wb = y; } }
  if (wa == wb) return nosplit();  // "homozygous"
  const uint64_t top1 = sv.v_hap[wa], top2 = sv.v_hap[wb];
  // ---- the assignment (:114-137): fewer agreements with the first haplotype -> group 0, more -> group 1, as many -> both groups, and the
  //      assignment alternates from 0 (the k-th such read of the kept list, k from 0, gets k % 2: a workgroup prefix carried across the rounds)
  uint32_t ties = 0, c0 = 0, c1 = 0;
  for (int base = 0; base < n; base += DW) {
    const int i = base + tid;
    const bool valid = i < n;
    int d1 = 0, d2 = 0;
    if (valid) { const uint64_t obs = prof[2 * i], val = prof[2 * i + 1]; d1 = __popcll(obs & ~(val ^ top1)); d2 = __popcll(obs & ~(val ^ top2)); }
    const bool tie = valid && d1 == d2;
    uint32_t tot;
    const uint32_t k = ties + cld::block_rank(tie, tot, red);
    if (valid) {
      const uint32_t gi = tie ? (k & 1u) : (d1 < d2 ? 0u : 1u);
      const bool in0 = gi == 0 || tie, in1 = gi == 1 || tie;
      grp[i] = (uint8_t)(gi | (tie ? 2u : 0u));
      sa.snv_read[r0 + i] = (uint8_t)((gi ? gt::SR_ASSIGN : 0) | (in0 ? gt::SR_IN0 : 0) | (in1 ? gt::SR_IN1 : 0));
      c0 += in0; c1 += in1;
    }
    ties += tot;
  }
  // (the barriers of the sums: every thread is done with the search's lists and sees grp and the bytes)
  const int cnt[2] = {(int)cld::block_sum_u32(c0, red), (int)cld::block_sum_u32(c1, red)};
  return end.split(cnt);
}

// How the search ends inside the deep size genotyper: the byte of the locus; a split goes on with deep_flank_tail, which fills the bytes
// of the search's lists next
struct DeepSizeEnd {
  DeepSize& sh; const DeepSnvArgs& sa; int64_t l; uint64_t r0; int n, nu;
  __device__ __forceinline__ bool nosplit() const { if (threadIdx.x == 0) sa.flank_done[l] = gt::FL_NOSPLIT | gt::FL_SNV; return false; }
  __device__ __forceinline__ bool handed(uint8_t why) const { if (threadIdx.x == 0) { sa.d.c.g.need_host[l] = 1; sa.flank_done[l] = (uint8_t)(gt::FL_HANDED | gt::FL_SNV | why); } return true; }
  __device__ __forceinline__ bool split(const int (&cnt)[2]) const {
    if (!deep_flank_tail<DeepSnvMembers>(sh, sa, l, r0, n, nu, cnt, sa.snv_read)) return nosplit();
    return true;
  }
};
__device__ __forceinline__ bool deep_snv_route(DeepSize& sh, const DeepSnvArgs& sa, int64_t l, uint64_t r0, int n, int nu) {
  DeepFlank& fl = deep_flank_lds(sh);
  DeepSizeEnd end{sh, sa, l, r0, n, nu};
  return deep_snv_search(*reinterpret_cast<DeepSnv*>(static_cast<void*>(fl.cnt)), reinterpret_cast<int32_t*>(sh.tmp), fl.grp, sh.red, sa, r0, n,
                         [&](int i) { return r0 + sa.d.sel_read[r0 + i]; }, end);
}

template <bool FLANK = false, bool SNV = false>
__global__ void __launch_bounds__(DW) deep_size_genotype_kernel(const DeepArgsOf<FLANK, SNV> aa) {
  static_assert(FLANK || !SNV, "the SNV forms are FLANK forms: they share the tail of the route and its LDS");
  __shared__ DeepSize sh;
  const DeepArgs& a = deep_of(aa);
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const gt::GtArgs& g = a.c.g;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  const uint64_t r0 = g.locus_read_begin[l];
  const int nr = (int)(g.locus_read_begin[l + 1] - r0);
  if (g.ploidy[l] == 0 || nr == 0 || nr > MAXR) return;  // (never on the list: what the one-wave kernel said stands)
  const int n = min((int)a.n_sel[k], nr);
  if (n == 0) { if (tid == 0) g.need_host[l] = 0; return; }  // no spanning read: the empty result stands
  for (int i = tid; i < n; i += DW) { sh.ln[i] = a.sel_len[r0 + i]; sh.off[i] = cld::seg_off(a, r0, i); }
  __syncthreads();
  // ---- unique lengths / counts ascending: rank sort of the lengths (thread t owns elements t, t + DW, ...), run boundaries, run lengths
  for (int i = tid; i < n; i += DW) {
    const uint32_t li = sh.ln[i];
    int rk = 0;
    for (int j = 0; j < n; ++j) { const uint32_t lj = sh.ln[j]; rk += (lj < li) || (lj == li && j < i); }
    sh.tmp[rk] = li;
  }
  __syncthreads();
  int u = 0;
  for (int base = 0; base < n; base += DW) {
    const int p = base + tid;
    const bool first = p < n && (p == 0 || sh.tmp[p - 1] != sh.tmp[p]);
    uint32_t total;
    const uint32_t q = (uint32_t)u + cld::block_rank(first, total, sh.red);
    if (first) { sh.ulen[q] = sh.tmp[p]; sh.ord[q] = (uint16_t)p; }
    u += (int)total;
  }
  __syncthreads();
  for (int q = tid; q < u; q += DW) sh.ucnt[q] = (uint32_t)(q + 1 < u ? (int)sh.ord[q + 1] : n) - (uint32_t)sh.ord[q];
  __syncthreads();
  const int ploidy = g.ploidy[l] == 1 ? 1 : 2;
  constexpr int NONE = 0x7FFFFFFF;
  // ---- diploid::genotype / haploid::genotype: candidates spread over the workgroup, each summed by one thread in ascending histogram
  //      order; the first minimum in candidate order wins
  double best_pen = __builtin_huge_val(); int best_p = NONE;
  if (ploidy == 2) {
    const int P = u * (u + 1) / 2;
    int si = 0, row0 = 0;  // row si of the candidate triangle starts at candidate row0 and has u - si entries
    for (int p = tid; p < P; p += DW) {
      while (p >= row0 + (u - si)) { row0 += u - si; ++si; }
      const int li = si + (p - row0);
      const uint32_t sa = sh.ulen[si], la = sh.ulen[li];
      const double max_frac = adiff_u(sa, la) <= 100 ? 0.25 : 0.05;
      double pen = 0.0;
      for (int i = 0; i < u; ++i) {
        const uint32_t ui = sh.ulen[i];
        const uint32_t st = ui != sa ? 10 + 2 * adiff_u(sa, ui) : 0, lt = ui != la ? 10 + 2 * adiff_u(la, ui) : 0;
        const double term = (double)(st < lt ? st : lt) + max_frac * (double)(st > lt ? st : lt);
        pen += term * (double)sh.ucnt[i];
      }
      if (best_p == NONE || pen < best_pen) { best_pen = pen; best_p = p; }
    }
  } else {
    for (int c = tid; c < u; c += DW) {
      const uint32_t uc = sh.ulen[c];
      double pen = 0.0;
      for (int i = 0; i < u; ++i) {
        const double term = sh.ulen[i] != uc ? 10.0 + 2.0 * (double)adiff_u(uc, sh.ulen[i]) : 0.0;
        pen += term * (double)sh.ucnt[i];
      }
      if (best_p == NONE || pen < best_pen) { best_pen = pen; best_p = c; }
    }
  }
  cld::block_min_vi(best_pen, best_p, sh.red);
  uint32_t size[2] = {0, 0}; int32_t civ[4] = {0, 0, 0, 0};
  int n_gt;
  if (ploidy == 2) {
    int si = 0, row0 = 0;
    while (best_p >= row0 + (u - si)) { row0 += u - si; ++si; }
    const int li = si + (best_p - row0);
    const uint32_t bs = sh.ulen[si], bl = sh.ulen[li];
    uint32_t short_size = bs < bl ? bs : bl, long_size = bs > bl ? bs : bl;
    if (short_size != long_size && u >= 2) {  // (uniform: every thread holds the same sizes)
      // the most frequent length, the first among equals (stable descending sort); the coverage is the number of kept reads
      double tv = 0.0; int top = NONE;
      for (int i = tid; i < u; i += DW) { const double v = -(double)sh.ucnt[i]; if (top == NONE || v < tv) { tv = v; top = i; } }
      cld::block_min_vi(tv, top, sh.red);
      const double top_frac = (double)sh.ucnt[top] / (double)(uint64_t)n;
      const uint32_t range = sh.ulen[u - 1] - sh.ulen[0];
      if (top_frac > 0.60 && range <= 6) short_size = long_size = sh.ulen[top];
    }
    n_gt = 2; size[0] = short_size; size[1] = long_size;
    uint32_t lo0 = short_size, hi0 = short_size, lo1 = long_size, hi1 = long_size;
    for (int i = tid; i < u; i += DW) {
      const uint32_t s = sh.ulen[i];
      if (adiff_u(s, short_size) <= adiff_u(s, long_size)) { lo0 = lo0 < s ? lo0 : s; hi0 = hi0 > s ? hi0 : s; }
      else { lo1 = lo1 < s ? lo1 : s; hi1 = hi1 > s ? hi1 : s; }
    }
    civ[0] = (int32_t)block_min_u32(lo0, sh.red); civ[1] = (int32_t)block_max_u32(hi0, sh.red);
    civ[2] = (int32_t)block_min_u32(lo1, sh.red); civ[3] = (int32_t)block_max_u32(hi1, sh.red);
  } else {
    n_gt = 1; size[0] = sh.ulen[best_p];
    civ[0] = (int32_t)sh.ulen[0]; civ[1] = (int32_t)sh.ulen[u - 1];
  }
  // ---- get_seq_hist: the kept reads in byte-lexicographic order of their segments, equal ones in read order (rank = #{smaller} +
  //      #{equal and earlier}); the first read of a run of equal segments represents it, as the insertion of the one-wave kernel does
  for (int i = tid; i < n; i += DW) {
    const uint8_t* pi = g.reads + sh.off[i]; const uint32_t li = sh.ln[i];
    uint32_t r = 0, eq = 1, dup = 0;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const int c = cmp_seg_thread(g.reads + sh.off[j], sh.ln[j], pi, li);
      r += (c < 0) || (c == 0 && j < i);
      eq += c == 0; dup |= (c == 0 && j < i);
    }
    sh.ord[r] = (uint16_t)i; sh.tmp[i] = eq | (dup << 31);
  }
  __syncthreads();
  int nu = 0;
  for (int base = 0; base < n; base += DW) {
    const int r = base + tid;
    const int i = r < n ? sh.ord[r] : 0;
    const bool first = r < n && !(sh.tmp[i] >> 31);
    uint32_t total;
    const uint32_t q = (uint32_t)nu + cld::block_rank(first, total, sh.red);
    if (first) { sh.u_rep[q] = (uint16_t)i; sh.u_cnt[q] = (uint16_t)(sh.tmp[i] & 0x7FFFFFFFu); }
    if constexpr (FLANK) { if (first) deep_flank_lds(sh).start[q] = (uint16_t)r; }
    nu += (int)total;
  }
  __syncthreads();
  // ---- FLANK: two sizes at most 10 apart (tr.rs:69-75) and tags that split the reads replace everything below; the size genotyper's
  //      own repair is not queued for such a locus
  if constexpr (SNV) {
    // ---- SNV: in the reference's order -- tags that split the reads own the locus (the tag route with both settings on; else the host
    //      finds the split as before: the byte stays 0), and only without such tags the SNVs of the flanks are tried
    if (n_gt == 2 && adiff_u(size[0], size[1]) <= 10) {
      int cnt[2];
      if (aa.hp_tag && deep_flank_assign(deep_flank_lds(sh).grp, a, aa.hp_tag, r0, n, cnt, sh.red)) {
        if (aa.tag_route) { deep_flank_tail<DeepTagMembers>(sh, aa, l, r0, n, nu, cnt); return; }
      } else if (deep_snv_route(sh, aa, l, r0, n, nu)) return;
    }
  } else if constexpr (FLANK) {
    if (aa.hp_tag && n_gt == 2 && adiff_u(size[0], size[1]) <= 10 && deep_flank_route(sh, aa, l, r0, n, nu)) return;
  }
  auto ulen_of = [&](int q) { return sh.ln[sh.u_rep[q]]; };
  // get_closest_len: the first length in sequence order at the smallest distance
  auto closest = [&](uint32_t target) {
    double bv = __builtin_huge_val(); int bq = NONE;
    for (int q = tid; q < nu; q += DW) { const double d = (double)adiff_u(ulen_of(q), target); if (d < bv) { bv = d; bq = q; } }
    cld::block_min_vi(bv, bq, sh.red);
    return ulen_of(bq == NONE ? 0 : bq);  // (nu >= 1: some thread has a value)
  };
  // get_most_frequent_seq: max_by_key takes the LAST maximum in sequence order: the largest (count, index) pair
  auto most_frequent = [&](uint32_t len) {
    double bv = __builtin_huge_val(); int bi = NONE;
    for (int q = tid; q < nu; q += DW) if (ulen_of(q) == len) { const double v = -(double)sh.u_cnt[q]; if (v <= bv) { bv = v; bi = -q; } }
    cld::block_min_vi(bv, bi, sh.red);
    return bi == NONE ? 0 : -bi;  // (len is the length of some unique sequence: some thread has a value)
  };
  int pick[2] = {most_frequent(closest(size[0])), -1};
  int n_pick = 1;
  if (n_gt != 1 && size[0] != size[1]) { pick[1] = most_frequent(closest(size[1])); n_pick = 2; }
  auto in_group = [&](int q, int al) {
    if (n_gt == 1) return true;
    const uint32_t d1 = adiff_u(ulen_of(q), size[0]), d2 = adiff_u(ulen_of(q), size[1]);
    return al == 0 ? d1 <= d2 : d2 < d1;
  };
  bool majority = true, lacks[2] = {false, false};
#pragma unroll
  for (int al = 0; al < 2; ++al) {  // split(): majority support of the pick inside its group, else stage B is needed
    if (al >= n_pick) break;
    uint32_t cov = 0;
    for (int q = tid; q < nu; q += DW) if (in_group(q, al)) cov += sh.u_cnt[q];
    const uint64_t coverage = cld::block_sum_u32(cov, sh.red), ref_count = in_group(pick[al], al) ? sh.u_cnt[pick[al]] : 0u;
    if (!(2 * ref_count >= coverage)) { majority = false; lacks[al] = true; }
  }
  if (majority) {
    const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0};
#pragma unroll
    for (int al = 0; al < 2; ++al) { if (al >= n_pick) break; const int rep = sh.u_rep[pick[al]]; ap[al] = g.reads + sh.off[rep]; aln[al] = sh.ln[rep]; }
    int n_al = n_pick;
    if (ploidy == 2 && n_al == 1) { ap[1] = ap[0]; aln[1] = aln[0]; n_al = 2; }
    // (a pick with majority support has the genotype's size)
    const bool ok = deep_size_write(a, l, r0, n, n_gt, n_al, ap, aln, civ, aln, sh.red);
    if (tid == 0) g.need_host[l] = ok ? 0 : 1;
    return;
  }
  // ---- stage B on the device: one vote group per allele without majority support, one alignment job per unique sequence of its group
  //      against the pick, in sequence order (job k of a group is its k-th member in that order)
  const gt::RepairBufs& rp = g.rp;
  bool can = rp.counts != nullptr;
  uint32_t nm[2] = {0, 0}, mbytes[2] = {0, 0};
  if (can) {
#pragma unroll
    for (int al = 0; al < 2; ++al) {
      if (al >= n_pick || !lacks[al]) continue;
      uint32_t cnt = 0, bytes = 0, over = ulen_of(pick[al]) > rp.max_seg;
      for (int q = tid; q < nu; q += DW) {
        if (!in_group(q, al)) continue;
        const uint32_t ln = ulen_of(q);
        over += ln > rp.max_seg; cnt += 1; bytes += ln;
      }
      nm[al] = cld::block_sum_u32(cnt, sh.red); mbytes[al] = cld::block_sum_u32(bytes, sh.red);
      if (cld::block_sum_u32(over, sh.red)) can = false;
    }
  }
  gt::GroupNeeds nd[2] = {};
  if (can) {
#pragma unroll
    for (int al = 0; al < 2; ++al) if (al < n_pick && lacks[al]) nd[al] = gt::group_needs(ulen_of(pick[al]), nm[al], mbytes[al], rp.vote_lds_pos);
    if (tid == 0) gt::repair_reserve(rp, l, g.n_loci, nm[0] + nm[1], (uint32_t)lacks[0] + (uint32_t)lacks[1], nd, sh.rsv);
    __syncthreads();
    can = sh.rsv.ok != 0;
  }
  if (!can) { if (tid == 0) g.need_host[l] = 1; return; }  // no room, a segment beyond max_seg, no device-side repair: the host path
  gt::Reserved at = sh.rsv;
  auto seg_of = [&](int q) { const int r = sh.u_rep[q]; return gt::Seg{sh.off[r], sh.ln[r]}; };  // of a unique sequence
  gt::RepairPend pd;
  pd.n_gt = n_gt; pd.n_pick = n_pick; pd.size[0] = size[0]; pd.size[1] = size[1];
  for (int q = 0; q < 4; ++q) pd.civ[q] = civ[q];
  pd.rep[0] = pd.rep[1] = -1; pd.grp[0] = pd.grp[1] = -1;
#pragma unroll
  for (int al = 0; al < 2; ++al) {
    if (al >= n_pick) break;
    pd.rep[al] = sh.u_rep[pick[al]];
    if (lacks[al]) pd.grp[al] = (int32_t)queue_group_scan(rp.groups, rp.jobs, at, seg_of(pick[al]), nm[al], nd[al], nu, [&, al](int q) { return in_group(q, al); }, seg_of, sh.red);
  }
  if (tid == 0) { rp.pend[l] = pd; g.need_host[l] = 2; }  // the locus waits for deep_size_finish_kernel
}

// ---- behind the consensus alignments and the column voting: the rest of genotype_size::genotype for the loci of the deep size list that
// wait for a repair (need_host = 2; they are in rp.loci too, where repair_finish_kernel passes them over by their read count).  A locus
// whose repaired allele does not fit (vote overflow, allele_cap) goes to the host path after all.
template <bool FLANK = false, bool SNV = false>
__global__ void __launch_bounds__(DW) deep_size_finish_kernel(const DeepArgsOf<FLANK, SNV> aa, const gt::FinishArgs f) {
  static_assert(FLANK || !SNV, "the SNV forms are FLANK forms");
  __shared__ Red red;
  const DeepArgs& a = deep_of(aa);
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const gt::GtArgs& g = a.c.g;
  const gt::RepairBufs& rp = g.rp;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  const bool waits = g.need_host[l] == 2;
  __syncthreads();  // (every thread has read the flag before thread 0 rewrites it below)
  if (!waits) return;
  const uint64_t r0 = g.locus_read_begin[l];
  const int nr = (int)(g.locus_read_begin[l + 1] - r0);
  const int n = min((int)a.n_sel[k], min(nr, MAXR));
  const gt::RepairPend pd = rp.pend[l];
  const int ploidy = g.ploidy[l] == 1 ? 1 : 2;
  auto seg_of = [&](int i) { return gt::Seg{cld::seg_off(a, r0, i), a.sel_len[r0 + i]}; };  // of a kept read
  if constexpr (FLANK) {
    // ... of a locus the haplotype-tag route left waiting (RP_FLANK): the alleles are the repaired sequences or the backbones of the tag
    // groups, smaller allele first (genotype_flank.rs:33-38); deep_size_write<BY_TAGS> recomputes the assignment from the tags (deterministic
    // from the same list of kept reads), which is the classification; its counts are num_spanning, the sizes are the allele lengths
    // (SNV forms, a record of the SNV route -- RP_SNV: the assignment is read back from DeepSnvArgs::snv_read instead, deep_size_write<BY_SNV>)
    if (pd.n_pick & gt::RP_FLANK) {
      uint8_t mark = 0;
      if constexpr (SNV) mark = pd.n_pick & gt::RP_SNV ? (uint8_t)gt::FL_SNV : (uint8_t)0;
      const uint8_t* tp[2] = {nullptr, nullptr}; uint32_t tl[2] = {0, 0};
      bool bad = n == 0;
#pragma unroll
      for (int t = 0; t < 2; ++t) if (!bad) bad = !gt::repaired_allele(pd, t, f, rp, g.reads, seg_of, tp[t], tl[t]);
      if (!bad) {
        const int sw = tl[0] > tl[1] ? 1 : 0;
        const uint8_t* sp[2] = {sw ? tp[1] : tp[0], sw ? tp[0] : tp[1]};
        const uint32_t sl[2] = {sw ? tl[1] : tl[0], sw ? tl[0] : tl[1]};
        const int32_t sc[4] = {sw ? pd.civ[2] : pd.civ[0], sw ? pd.civ[3] : pd.civ[1], sw ? pd.civ[0] : pd.civ[2], sw ? pd.civ[1] : pd.civ[3]};
        if constexpr (SNV) bad = mark ? !deep_size_write<BY_SNV>(a, l, r0, n, 2, 2, sp, sl, sc, sl, red, aa.hp_tag, sw, aa.snv_read) : !deep_size_write<BY_TAGS>(a, l, r0, n, 2, 2, sp, sl, sc, sl, red, aa.hp_tag, sw);
        else bad = !deep_size_write<BY_TAGS>(a, l, r0, n, 2, 2, sp, sl, sc, sl, red, aa.hp_tag, sw);
      }
      if (tid == 0) {
        if (bad) { g.need_host[l] = 1; aa.flank_done[l] = (uint8_t)(gt::FL_HANDED | mark); }
        else { g.skip_b[l] = 0; if (g.finish_clears_need) g.need_host[l] = 0; aa.flank_done[l] = (uint8_t)(gt::FL_DONE | gt::FL_REPAIRED | mark); }
      }
      return;
    }
  }
  // the alleles: the repaired sequence of a group, or the pick that had majority support
  const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0};
  bool fail = n == 0;
#pragma unroll
  for (int al = 0; al < 2; ++al) if (al < pd.n_pick && !fail) fail = !gt::repaired_allele(pd, al, f, rp, g.reads, seg_of, ap[al], aln[al]);
  int n_al = pd.n_pick;
  if (!fail && ploidy == 2 && n_al == 1) { ap[1] = ap[0]; aln[1] = aln[0]; n_al = 2; }
  if (!fail) fail = !deep_size_write(a, l, r0, n, pd.n_gt, n_al, ap, aln, pd.civ, pd.size, red);
  if (fail) { if (tid == 0) g.need_host[l] = 1; return; }
  // (need_host stays 2 unless one HMM batch runs behind the repair: see repair_finish_kernel)
  if (tid == 0) { g.skip_b[l] = 0; if (g.finish_clears_need) g.need_host[l] = 0; }
}

}  // namespace gtd
}  // namespace trgt
