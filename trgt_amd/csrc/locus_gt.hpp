// trgt_amd/csrc/locus_gt.hpp -- the host glue of analyze_tr on the device, for the common case:
//   get_spanning_reads  (src/trgt/workflows/tr.rs:111-184)  filter, stable sort by span length, uniform downsample
//   genotype_size::genotype (genotype_size.rs:6-64) with diploid::genotype (diploid.rs:5-103) / haploid::genotype
//   (haploid.rs:3-30), consensus::get_consensus (consensus.rs:113-154), the read classification (genotype_size.rs:42-61)
//   and "reference allele first" (tr.rs:95-101).
// One wavefront per locus; everything the decisions depend on (span lengths, the repeat segments themselves) is staged in
// LDS (segments beyond GT_SEG_LDS bytes are compared where they lie, in the read blob).  A locus of more than GT_MAX_READS reads is out of
// this kernel's envelope and leaves it with need_host = 1: on a context that opted in (trgt_hip_set_size_max_reads) the workgroup-wide
// kernels of locus_gt_deep.hpp then take it, up to 2 048 reads, and overwrite that mark; otherwise, and beyond that, the host path of
// locus.hip.  A locus whose pick lacks majority support waits (need_host = 2) for the consensus alignments of stage B
// (repair_consensus, consensus.rs:5-111) and repair_finish_kernel below, or goes to the host path when that chain has no room for it.
// The arithmetic (f64 penalties, tie-breaks) is written operation for operation like the host version in locus.hip, which the oracle pins.
// The FLANK instantiations (contexts that opted in, trgt_hip_set_flank_device) also run the haplotype-tag branch of
// genotype_flank::genotype (genotype_flank.rs:9-76, 147-170; tr.rs:69-75) for a locus whose two sizes are at most 10 apart: see flank_route.
// The SNV instantiations (contexts that opted in, trgt_hip_set_snv_split_device; batches that carry mismatch offsets) add the other branch,
// the split by heterozygous SNVs of the flanks (genotype_flank.rs:78-138, 171-290): see snv_route.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "repair_queue.hpp"

namespace trgt {
namespace gt {

// Two instantiations: <256, 16 KB> and, for batches whose loci all have at most 64 reads, <64, 8 KB> -- 11 instead of 27 KB of LDS
// per locus, i.e. 14 instead of 5 loci in flight per CU for a kernel that is all latency (0.53 -> 0.3 ms on the 10k-locus batch).
constexpr int GT_MAX_READS = 256;      // reads of a locus (and therefore kept spanning reads) handled by the large instantiation
constexpr int GT_SEG_LDS = 16 * 1024;  // bytes of repeat segments staged per locus (large instantiation)

// ---- consensus repair on the device (genotype_size.rs:32-37 -> utils::align -> repair_consensus, consensus.rs:5-111): a locus whose pick
// lacks majority support no longer goes back to the host.  The genotyper writes the consensus alignments it needs (backbone = the pick,
// texts = the unique sequences of the allele's group, all of them segments of the read blob) into a job list, one vote group per allele
// and a record of what it had decided; behind it run the alignment kernel over that list, the column voting and repair_finish_kernel,
// which classifies the reads against the repaired alleles and writes the locus out.  The records, the reservation of space and the job
// writer are those of repair_queue.hpp, shared with every other route; a locus that finds no room (or is out of the envelope: a segment
// longer than max_seg) takes the host path as before.
// n_pick of a record the haplotype-tag route wrote (FLANK instantiations only): rep[] are the backbones of the two tag groups, civ[] the
// groups' length ranges, and the finish is flank_finish's
constexpr int32_t RP_FLANK = 0x100;
constexpr int32_t RP_SNV = 0x200;  // with RP_FLANK: the groups are the SNV branch's (SNV instantiations only)
// GtFlankArgs::flank_done, per locus: the tag split replaced the genotype (FL_DONE; FL_DONE | FL_REPAIRED: behind the repair chain), or the
// split was accepted and the locus handed to the host path (no room in the chain, a segment beyond max_seg, allele_cap)
// The SNV instantiations add: FL_NOSPLIT -- the kernel evaluated both branches of genotype_flank for the locus and neither splits its reads
// (the host need not look again); FL_SNV -- the byte is the SNV branch's (its loci are counted by trgt_hip_snv_split_stats and by no other
// count); FL_UNDECIDED, with FL_HANDED -- handed to the host path because the candidate search was not decided beyond the margin
enum { FL_DONE = 1, FL_REPAIRED = 2, FL_HANDED = 4, FL_NOSPLIT = 8, FL_SNV = 16, FL_UNDECIDED = 32 };
// limits of the SNV branch on the device; a locus beyond one of them is handed to the host path (FL_HANDED | FL_SNV)
constexpr int SNV_MAX_SNVS = 64;        // called SNVs: one bit each in the two masks of a read's profile
constexpr int SNV_MAX_HAPS = 16;        // distinct fully observed profiles: 136 candidate genotypes, three rounds of one lane per candidate
constexpr int SNV_OFFS_PER_READ = 8;    // in-region mismatch offsets of a locus (occurrences, all reads together): 8 * MAXR.  They are counted
                                        // all against all: at the cap every lane compares its 8 * MAXR / 64 entries with 8 * MAXR others,
                                        // (8 * MAXR)^2 / 64 LDS reads per lane -- 4 096 for MAXR = 64, 65 536 for MAXR = 256
// the per-read byte of a locus the SNV branch left waiting for the repair chain (SnvArgs::snv_read): assignment, membership of either group
enum { SR_ASSIGN = 1, SR_IN0 = 2, SR_IN1 = 4 };

// GtArgs::finish_clears_need as locus_genotype_kernel reads it.  GT_DEV_SERIAL (TRGT_GT_SERIAL, developer build): every section of the size
// genotyper as one lane, or the whole wave in step, takes it read by read; GT_DEV_WEAK_HASH (TRGT_GT_WEAK_HASH): gt_equal_reads tells
// sequences apart by length alone
enum { GT_DEV_SERIAL = 2, GT_DEV_WEAK_HASH = 4 };
struct GtArgs {
  const uint8_t* reads; const uint64_t* read_off; const uint32_t* read_len; const uint64_t* locus_read_begin;
  const int32_t* span_start; const int32_t* span_end;
  const uint8_t* ploidy; const uint8_t* tr_blob; const uint64_t* tr_off; const uint32_t* tr_len;
  const uint64_t* allele_off; const uint32_t* allele_cap;
  int64_t n_loci; int32_t flank_len, max_depth;
  uint8_t* need_host; int32_t* n_alleles; uint8_t* allele_blob; uint32_t* allele_len; int32_t* ci; int32_t* num_spanning;
  int32_t* classification; int32_t* read_rank; uint32_t* n_spanning_reads;
  uint8_t* flipped;  // per locus: the two alleles were swapped to put the reference allele first
  int32_t* gt_size;  // [2 n_loci] TrSize::size of the genotype behind every allele (optional)
  const uint8_t* genotyper;  // optional [n_loci]: 1 = Genotyper::Cluster, a locus the host genotypes (need_host = 1 at once)
  uint8_t* skip_b;   // [n_loci] 0 for the loci repair_finish_kernel completed (their HMM batch runs behind it), else 1
  int32_t finish_clears_need;  // the finish kernels: 1 = repair_finish_kernel also sets need_host = 0 (nothing reads it concurrently: one HMM batch behind the repair);
                               // locus_genotype_kernel, launched before that is decided: its developer switches (GT_DEV_*; the struct must not grow)
  RepairBufs rp;
  // calls with filter_impure_trs on (locus_purity.hpp), read by the PRESEL instantiations only: the kept reads of locus l, already selected,
  // ordered and filtered, in slots [locus_read_begin[l], + n_sel[l]) -- read (index inside the locus), span start, span length
  const uint32_t *sel_read, *sel_start, *sel_len, *n_sel;
};
// The arguments of the FLANK instantiations (contexts that opted in to the tag split on the device).  A struct of its own: GtArgs is part
// of the arguments of every cluster and deep kernel, whose register allocation follows its size.
struct GtFlankArgs : GtArgs {
  const int16_t* hp_tag;  // per read of the batch: the HP tag (-1 = None)
  uint8_t* flank_done;    // [n_loci] FL_* above
};
// The arguments of the SNV instantiations (contexts that opted in to the SNV split on the device, batches with mismatch offsets).
struct SnvArgs : GtFlankArgs {
  const int32_t *start_offset, *end_offset;  // per read of the batch (NULL = 0 for every read, as in flank_split)
  const int32_t* mismatch_offsets; const uint64_t* mismatch_off;  // per read r: its ascending offsets in [mismatch_off[r], mismatch_off[r + 1])
  uint8_t* snv_read;      // per read slot of the batch, by position in the kept list: SR_* of a locus that waits for the repair chain
  double ln_match, ln_mis, ln2;  // ln 0.9, ln(1.0 - 0.9), ln 2 as the host's libm rounds them
  int32_t tag_route;      // 1: tags that split the reads are flank_route's (trgt_hip_set_flank_device is on as well); 0: such a locus is the host's
};
template <bool FLANK, bool SNV = false> using GtArgsOf = std::conditional_t<SNV, SnvArgs, std::conditional_t<FLANK, GtFlankArgs, GtArgs>>;

// what the haplotype-tag route adds to the LDS of the FLANK instantiations (1.5 KB for 256 reads); the assignment lives in cls[]
template <int MAXR, bool FLANK> struct FlankShared {};
template <int MAXR> struct FlankShared<MAXR, true> {
  uint16_t f_uidx[MAXR];    // per kept read: its unique sequence -- first the position of the first read that carries it, then its rank in u_rep
  uint16_t f_cnt[2][MAXR];  // multiplicity of every unique sequence inside either tag group
  uint32_t f_med[2][2];     // the two middle lengths of either group
};
// ... and the SNV branch (10.9 KB for 256 reads, 3 KB for 64): offsets of the reads, the in-region mismatch offsets while the SNVs are
// called and -- in the same bytes, the offsets being done with -- the profiles, the candidates' haplotypes and log-likelihoods
template <int MAXR, bool SNV> struct SnvShared {};
template <int MAXR> struct SnvShared<MAXR, true> {
  int32_t v_so[MAXR], v_eo[MAXR];  // per kept read: start_offset / end_offset
  union {
    int32_t offs[SNV_OFFS_PER_READ * MAXR];         // the in-region offsets of all reads, in read order
    struct { uint64_t obs[MAXR], val[MAXR]; } p;  // per kept read: SNV k is bit k of obs (the read covers it) and of val (it carries the mismatch)
  } v;
  int32_t v_snv[SNV_MAX_SNVS], v_tmp[SNV_MAX_SNVS];  // the called SNVs ascending (v_tmp: as found)
  uint64_t v_hap[SNV_MAX_HAPS];                      // the distinct fully observed profiles in the derived order of Option<bool>
  double v_ll[SNV_MAX_HAPS * (SNV_MAX_HAPS + 1) / 2];
  uint8_t v_tie[MAXR];                               // per kept read: it agrees equally with both haplotypes and belongs to both groups
  int32_t v_reg[2];
};
template <int MAXR, int SEG, bool FLANK = false, bool SNV = false>
struct GtShared : FlankShared<MAXR, FLANK>, SnvShared<MAXR, SNV> {
  uint32_t r_s[MAXR], r_len[MAXR];     // per read of the locus: span start / span length (0xFFFFFFFF start = not kept)
  uint64_t r_off[MAXR];                        // per read: byte offset of the read in the blob
  uint32_t s_read[MAXR], s_start[MAXR], s_len[MAXR];  // kept reads in LocusResult.reads order
  uint16_t s_loff[MAXR];                                              // offset of the segment bytes in `bytes` (4-aligned)
  uint16_t u_rep[MAXR], u_cnt[MAXR];  // unique sequences (lexicographic order): representative, multiplicity
  uint32_t ulen[MAXR], ucnt[MAXR];    // unique lengths ascending, multiplicities
  int8_t cls[MAXR];
  int n, n_sizes, bail, fits;
  // decisions of lane 0, written out by the whole wave
  int res_n_gt, res_flip, res_rep[2], res_ci[4], res_hap[2];
  Reserved rsv;  // device-side repair: the reservation of lane 0
  uint32_t ref_off;                                    // the reference repeat staged behind the segments
  alignas(16) uint8_t bytes[SEG];
};

__device__ __forceinline__ uint32_t adiff_u(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

// cmp_seg of locus.hip (memcmp over the common prefix, then the shorter one first) on 4-aligned LDS copies, by the whole wave:
// lane i compares dword i (64 dwords per round), a ballot finds the first difference; byte order is memory order, so the
// deciding dwords are compared byte-swapped.  Uniform arguments, uniform result.
__device__ __forceinline__ int cmp_lds(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
  const int lane = threadIdx.x & 63;
  const uint32_t m = na < nb ? na : nb;
  const uint32_t* A = reinterpret_cast<const uint32_t*>(a); const uint32_t* B = reinterpret_cast<const uint32_t*>(b);
  const uint32_t nw = (m + 3u) >> 2;
  for (uint32_t base = 0; base < nw; base += 64) {
    const uint32_t w = base + (uint32_t)lane;
    uint32_t x = 0, y = 0;
    if (w < nw) {
      x = A[w]; y = B[w];
      if (w == nw - 1 && (m & 3u)) { const uint32_t mask = (1u << (8 * (m & 3u))) - 1u; x &= mask; y &= mask; }
    }
    const unsigned long long ne = __ballot(x != y);
    if (ne) {
      const int f = __ffsll((long long)ne) - 1;
      const uint32_t xf = (uint32_t)__builtin_amdgcn_readlane((int)x, f), yf = (uint32_t)__builtin_amdgcn_readlane((int)y, f);
      return __builtin_bswap32(xf) < __builtin_bswap32(yf) ? -1 : 1;
    }
  }
  return na < nb ? -1 : (na > nb ? 1 : 0);
}

// the same order on byte strings anywhere (global memory, any alignment): lane i assembles dword i from four byte loads.  For the
// loci whose repeat segments do not fit the LDS staging area (long alleles, deep loci): a few per cent of a genome-wide catalog.
__device__ __forceinline__ int cmp_bytes(const uint8_t* __restrict__ a, uint32_t na, const uint8_t* __restrict__ b, uint32_t nb) {
  const int lane = threadIdx.x & 63;
  const uint32_t m = na < nb ? na : nb;
  for (uint32_t base = 0; base < m; base += 256) {
    uint32_t x = 0, y = 0;  // big-endian: the first byte is the most significant
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t i = base + 4u * (uint32_t)lane + q;
      if (i < m) { x |= (uint32_t)a[i] << (24 - 8 * q); y |= (uint32_t)b[i] << (24 - 8 * q); }
    }
    const unsigned long long ne = __ballot(x != y);
    if (ne) {
      const int f = __ffsll((long long)ne) - 1;
      const uint32_t xf = (uint32_t)__builtin_amdgcn_readlane((int)x, f), yf = (uint32_t)__builtin_amdgcn_readlane((int)y, f);
      return xf < yf ? -1 : 1;
    }
  }
  return na < nb ? -1 : (na > nb ? 1 : 0);
}

// 16 lanes copy n bytes from global (any alignment) to a 4-aligned LDS destination, 16 bytes per lane and round
__device__ __forceinline__ void copy16(uint8_t* dst, const uint8_t* __restrict__ src, uint32_t n, int sub) {
  const uint32_t full = n >> 4;
  for (uint32_t w = sub; w < full; w += 16) {
    uint4 v; __builtin_memcpy(&v, src + 16 * w, 16);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst) + 4 * w;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  for (uint32_t b = full * 16 + (uint32_t)sub; b < n; b += 16) dst[b] = src[b];
}

// get_spanning_reads (tr.rs:111-184) for one locus by one wave: filter, stable sort by span length, uniform downsample.  On return
// sh.n kept reads sit in sh.s_read / s_start / s_len in LocusResult.reads order (sh.r_off: blob offsets of all reads of the locus).
template <int MAXR, class SH>
__device__ __forceinline__ void gt_front(SH& sh, const GtArgs& a, uint64_t r0, int nr, int lane) {
  const int F = a.flank_len;
  for (int i = lane; i < nr; i += 64) {
    const int32_t s = a.span_start[r0 + i], e = a.span_end[r0 + i];
    const bool keep = s >= 0 && s >= F && (int64_t)a.read_len[r0 + i] - e >= F;  // filter of get_spanning_reads (tr.rs:139-145)
    sh.r_s[i] = keep ? (uint32_t)s : 0xFFFFFFFFu; sh.r_len[i] = keep ? (uint32_t)(e - s) : 0u;
    sh.r_off[i] = a.read_off[r0 + i];
  }
  __syncthreads();
  if (lane == 0) {  // in read order
    int n = 0;
    for (int i = 0; i < nr; ++i)
      if (sh.r_s[i] != 0xFFFFFFFFu) { sh.s_read[n] = (uint32_t)i; sh.s_start[n] = sh.r_s[i]; sh.s_len[n] = sh.r_len[i]; ++n; }
    sh.n = n;
  }
  __syncthreads();
  const int n = sh.n;
  if (n > 0) {
    // ---- stable sort by span length (:157): rank = #{shorter} + #{equal and earlier}; every lane owns elements lane, lane+64, ...
    {
      uint32_t rd[MAXR / 64], st[MAXR / 64], ln[MAXR / 64]; int rk[MAXR / 64];
      for (int t = 0; t < MAXR / 64; ++t) {
        const int i = lane + 64 * t;
        rk[t] = -1;
        if (i < n) {
          rd[t] = sh.s_read[i]; st[t] = sh.s_start[i]; ln[t] = sh.s_len[i];
          int r = 0;
          for (int j = 0; j < n; ++j) { const uint32_t lj = sh.s_len[j]; r += (lj < ln[t]) || (lj == ln[t] && j < i); }
          rk[t] = r;
        }
      }
      __syncthreads();
      for (int t = 0; t < MAXR / 64; ++t)
        if (rk[t] >= 0) { sh.s_read[rk[t]] = rd[t]; sh.s_start[rk[t]] = st[t]; sh.s_len[rk[t]] = ln[t]; }
      __syncthreads();
    }
    if (lane == 0) {
      // ---- uniform downsample (:172-184), sequential swaps exactly as written there
      if (n > a.max_depth) {
        const double step = (double)n / (double)a.max_depth;
        double fast = 0.0;
        for (int i = 0; i < a.max_depth; ++i) {
          const int ind = (int)floor(fast);
          if (ind != i) {
            const uint32_t t0 = sh.s_read[i], t1 = sh.s_start[i], t2 = sh.s_len[i];
            sh.s_read[i] = sh.s_read[ind]; sh.s_start[i] = sh.s_start[ind]; sh.s_len[i] = sh.s_len[ind];
            sh.s_read[ind] = t0; sh.s_start[ind] = t1; sh.s_len[ind] = t2;
          }
          fast += step;
        }
        sh.n = a.max_depth;
      }
    }
    __syncthreads();
  }
}

// The kept reads of a locus for every kernel behind the selection: gt_front, or -- PRESEL, the instantiations launched when
// filter_impure_trs is on -- the list purity_select_kernel and purity_filter_kernel (locus_purity.hpp) left in global memory.  Either
// way sh.n kept reads sit in sh.s_read / s_start / s_len in LocusResult.reads order and sh.r_off holds the blob offsets of all reads.
template <int MAXR, bool PRESEL, class SH>
__device__ __forceinline__ void gt_selected(SH& sh, const GtArgs& a, int64_t l, uint64_t r0, int nr, int lane) {
  if constexpr (!PRESEL) gt_front<MAXR>(sh, a, r0, nr, lane);
  else {
    const int n = min((int)a.n_sel[l], nr);
    for (int i = lane; i < nr; i += 64) sh.r_off[i] = a.read_off[r0 + i];
    for (int i = lane; i < n; i += 64) { sh.s_read[i] = a.sel_read[r0 + i]; sh.s_start[i] = a.sel_start[r0 + i]; sh.s_len[i] = a.sel_len[r0 + i]; }
    if (lane == 0) sh.n = n;
    __syncthreads();
  }
}

// ---- the haplotype-tag branch of genotype_flank::genotype on the device (genotype_flank.rs:9-76; applied by analyze at tr.rs:69-75 to a
// diploid locus whose two sizes are at most 10 apart).  The SNV-clustering branch (:78-138) stays on the host: a locus whose tags do not
// split its reads leaves the kernels with the length genotype, and the host tries that branch for it as before.
__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) { for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o); v = w < v ? w : v; } return v; }
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) { for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o); v = w > v ? w : v; } return v; }

// get_trs_with_hp (:43-76) over the kept reads in sh.s_read order: tag 1 -> group 0, tag 2 -> group 1, every other read alternates (the
// k-th untagged read, k from 0, goes to group k % 2: assignment_tie_breaker starts at 1 and is advanced before use).  64 reads per round:
// a ballot of the untagged lanes and the count of those below a lane give k.  Leaves the assignment in sh.cls and the group sizes in
// cnt; true when the split is accepted (both groups occur, at least 70 % of the reads tagged).  Uniform arguments, uniform result.
template <class SH>
__device__ __forceinline__ bool flank_assign(SH& sh, const int16_t* __restrict__ hp, uint64_t r0, int n, int lane, int cnt[2]) {
  int untagged = 0;
  cnt[0] = cnt[1] = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const int tag = i < n ? (int)hp[r0 + sh.s_read[i]] : 0;
    const bool un = i < n && tag != 1 && tag != 2;
    const unsigned long long ub = __ballot(un);
    const int k = untagged + __popcll(ub & ((1ull << lane) - 1ull));
    const int g = un ? (k & 1) : tag - 1;
    if (i < n) sh.cls[i] = (int8_t)g;
    const int ones = __popcll(__ballot(i < n && g == 1));
    cnt[1] += ones; cnt[0] += (n - base < 64 ? n - base : 64) - ones;
    untagged += __popcll(ub);
  }
  __syncthreads();
  return cnt[0] > 0 && cnt[1] > 0 && (double)(n - untagged) / (double)n >= 0.7;
}

// Who belongs to group g of a split whose assignment is in sh.cls.  By tags: the reads assigned to it.  By SNVs (:114-137): those, and the
// reads that agree equally with both haplotypes (sh.v_tie), which join both groups while their assignment alternates.
struct TagMembers { static constexpr bool BOTH = false; template <class SH> static __device__ __forceinline__ bool in(const SH& sh, int i, int g) { return sh.cls[i] == g; } };
struct SnvMembers { static constexpr bool BOTH = true; template <class SH> static __device__ __forceinline__ bool in(const SH& sh, int i, int g) { return sh.cls[i] == g || sh.v_tie[i]; } };

// What follows an accepted split (genotype_flank.rs:20-41), behind get_seq_hist (nu unique sequences in sh.u_rep, sh.f_uidx[i] = position
// of the first read with read i's sequence): simple_consensus (:147-170) of either group -- cnt[g] members, MEM says who; hap[g] reads are
// assigned to it (num_spanning, tr.rs:79-82).  Without a group below 50 % the genotype is written to sh.res_* / sh.cls like the length
// genotyper's, else the groups join the call's repair chain (sh.bail = 2: flank_finish completes the locus), or the locus is handed to
// the host path (sh.bail = 1).  mark: FL_SNV for the SNV branch, 0 for the tags'.  false (BOTH only): a group is empty, there is no split.
// Called by the whole wave with uniform arguments.
template <class MEM, class SH>
__device__ __forceinline__ bool flank_tail(SH& sh, const GtFlankArgs& a, int64_t l, int n, int nu, int lane, bool fits, uint32_t refn, uint64_t refo, const int cnt[2],
                                           const int hap[2], const uint8_t mark) {
  if constexpr (MEM::BOTH) { if (cnt[0] == 0 || cnt[1] == 0) return false; }
  // ---- the unique sequence of every read as its rank in u_rep (the insertions of get_seq_hist moved the ranks while the list grew)
  uint16_t* inv = sh.f_cnt[0];
  for (int q = lane; q < nu; q += 64) inv[sh.u_rep[q]] = (uint16_t)q;
  __syncthreads();
  for (int i = lane; i < n; i += 64) sh.f_uidx[i] = inv[sh.f_uidx[i]];
  __syncthreads();
  // ---- multiplicities inside the groups (lane q owns unique sequence q), and the middle lengths of either group by rank
  for (int q = lane; q < nu; q += 64) {
    int c0 = 0, c1 = 0;
    if constexpr (MEM::BOTH) { for (int i = 0; i < n; ++i) if (sh.f_uidx[i] == q) { c0 += MEM::in(sh, i, 0); c1 += MEM::in(sh, i, 1); } }
    else for (int i = 0; i < n; ++i) if (sh.f_uidx[i] == q) { if (sh.cls[i]) ++c1; else ++c0; }
    sh.f_cnt[0][q] = (uint16_t)c0; sh.f_cnt[1][q] = (uint16_t)c1;
  }
  auto middle = [&](int i, int g) {  // read i is a middle element of group g: its rank among the group's lengths
    const uint32_t li = sh.s_len[i];
    int r = 0;
    for (int j = 0; j < n; ++j) { const uint32_t lj = sh.s_len[j]; r += MEM::in(sh, j, g) && (lj < li || (lj == li && j < i)); }
    if (r == cnt[g] / 2) sh.f_med[g][1] = li;
    if (r == cnt[g] / 2 - 1) sh.f_med[g][0] = li;
  };
  for (int i = lane; i < n; i += 64) {
    if constexpr (MEM::BOTH) { for (int g = 0; g < 2; ++g) if (MEM::in(sh, i, g)) middle(i, g); }
    else middle(i, sh.cls[i]);
  }
  __syncthreads();
  int rep[2]; uint32_t aln[2], lo[2], hi[2]; bool lacks[2];
  for (int g = 0; g < 2; ++g) {
    // utils::math::median (math.rs:73-98) as f32, truncated: the middle value, or (a + b) as i32, then / 2.0
    const float med = (cnt[g] & 1) ? (float)(int32_t)sh.f_med[g][1] : (float)((int32_t)sh.f_med[g][0] + (int32_t)sh.f_med[g][1]) / 2.0f;
    const uint32_t median_len = (uint32_t)med;
    uint32_t top = 0, mn = 0xFFFFFFFFu, mx = 0;
    for (int q = lane; q < nu; q += 64) top = sh.f_cnt[g][q] > top ? sh.f_cnt[g][q] : top;
    top = wave_max_u(top);
    // among the sequences with the largest multiplicity, in u_rep order: the first minimum of |len - median|
    uint32_t bd = 0xFFFFFFFFu; int bq = 0x7FFFFFFF;
    for (int q = lane; q < nu; q += 64)
      if (sh.f_cnt[g][q] == top) { const uint32_t d = adiff_u(sh.s_len[sh.u_rep[q]], median_len); if (d < bd) { bd = d; bq = q; } }
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t od = (uint32_t)__shfl_xor((int)bd, o); const int oq = __shfl_xor(bq, o);
      if (od < bd || (od == bd && oq < bq)) { bd = od; bq = oq; }
    }
    for (int i = lane; i < n; i += 64) if (MEM::in(sh, i, g)) { mn = sh.s_len[i] < mn ? sh.s_len[i] : mn; mx = sh.s_len[i] > mx ? sh.s_len[i] : mx; }
    lo[g] = wave_min_u(mn); hi[g] = wave_max_u(mx);
    rep[g] = sh.u_rep[bq]; aln[g] = sh.s_len[rep[g]];
    lacks[g] = (double)top / (double)cnt[g] < 0.5;
  }
  if (lacks[0] || lacks[1]) {
    // ---- a group below 50 %: backbone = its sequence, one member per read of the group in read order, duplicates included
    const RepairBufs& rp = a.rp;
    bool can = rp.counts != nullptr;
    uint32_t nm[2] = {0, 0}; unsigned long long mbytes[2] = {0, 0};
    if (can)
      for (int g = 0; g < 2; ++g) {
        if (!lacks[g]) continue;
        if (aln[g] > rp.max_seg) can = false;
        for (int i = 0; i < n; ++i) {
          if (!MEM::in(sh, i, g)) continue;
          if (sh.s_len[i] > rp.max_seg) can = false;
          nm[g] += 1; mbytes[g] += sh.s_len[i];
        }
      }
    GroupNeeds nd[2] = {};
    if (can) {
#pragma unroll
      for (int g = 0; g < 2; ++g) if (lacks[g]) nd[g] = group_needs(aln[g], nm[g], mbytes[g], rp.vote_lds_pos);
      if (lane == 0) repair_reserve(rp, l, a.n_loci, nm[0] + nm[1], (uint32_t)lacks[0] + (uint32_t)lacks[1], nd, sh.rsv);
      __syncthreads();
      can = sh.rsv.ok != 0;
    }
    if (!can) { sh.bail = 1; if (lane == 0) a.flank_done[l] = FL_HANDED | mark; return true; }
    Reserved at = sh.rsv;
    auto seg_of = [&](int i) { return Seg{sh.r_off[sh.s_read[i]] + sh.s_start[i], sh.s_len[i]}; };
    RepairPend pd;
    pd.n_gt = 2; pd.n_pick = 2 | RP_FLANK | (MEM::BOTH ? RP_SNV : 0); pd.size[0] = aln[0]; pd.size[1] = aln[1];
    for (int g = 0; g < 2; ++g) { pd.civ[2 * g] = (int32_t)lo[g]; pd.civ[2 * g + 1] = (int32_t)hi[g]; pd.rep[g] = rep[g]; pd.grp[g] = -1; }
#pragma unroll
    for (int g = 0; g < 2; ++g)
      if (lacks[g]) pd.grp[g] = (int32_t)queue_group<64>(rp.groups, rp.jobs, at, seg_of(rep[g]), nm[g], nd[g], n, [&, g](int i) { return MEM::in(sh, i, g); }, seg_of);
    if (lane == 0) rp.pend[l] = pd;
    sh.bail = 2;  // the locus waits for repair_finish_kernel
    return true;
  }
  // ---- both groups have their sequence: smaller allele first (:33-38: alleles and intervals swap, the assignment flips), the
  //      assignment is the classification, then reference allele first (tr.rs:95-101)
  const int sw = aln[0] > aln[1] ? 1 : 0;
  if (sw) for (int i = lane; i < n; i += 64) sh.cls[i] = (int8_t)(1 - sh.cls[i]);
  auto seg_glob = [&](int i) { return a.reads + sh.r_off[sh.s_read[i]] + sh.s_start[i]; };
  auto eq_ref = [&](int g) {
    return fits ? cmp_lds(sh.bytes + sh.s_loff[rep[g]], aln[g], sh.bytes + sh.ref_off, refn) == 0 : cmp_bytes(seg_glob(rep[g]), aln[g], a.tr_blob + refo, refn) == 0;
  };
  int order[2] = {sw, 1 - sw}; int flip = 0;
  if (!eq_ref(order[0]) && eq_ref(order[1])) { order[0] = 1 - sw; order[1] = sw; flip = 1; }
  if (aln[0] > a.allele_cap[l] || aln[1] > a.allele_cap[l]) { sh.bail = 1; if (lane == 0) a.flank_done[l] = FL_HANDED | mark; return true; }  // the host path reports the error
  sh.res_n_gt = 2; sh.res_flip = flip;
  for (int oi = 0; oi < 2; ++oi) {
    const int g = order[oi];
    sh.res_rep[oi] = rep[g]; sh.res_ci[2 * oi] = (int)lo[g]; sh.res_ci[2 * oi + 1] = (int)hi[g]; sh.res_hap[oi] = hap[g];
  }
  if (lane == 0) a.flank_done[l] = FL_DONE | mark;
  return true;
}

// The tag route inside the genotype kernel.  false: the tags do not split the reads and the locus continues with the length genotype (or,
// SNV forms, with snv_route).  true: the locus is settled by flank_tail.
template <class SH>
__device__ __forceinline__ bool flank_route(SH& sh, const GtFlankArgs& a, int64_t l, uint64_t r0, int n, int nu, int lane, bool fits, uint32_t refn, uint64_t refo) {
  int cnt[2];
  if (!flank_assign(sh, a.hp_tag, r0, n, lane, cnt)) return false;
  return flank_tail<TagMembers>(sh, a, l, n, nu, lane, fits, refn, refo, cnt, cnt, (uint8_t)0);
}

// ---- the SNV branch of genotype_flank::genotype on the device (get_trs_with_clustering, genotype_flank.rs:78-138, with get_analysis_region,
// call_snvs, the profiles, the candidate genotypes and their log-likelihoods, :171-290), tried where the tags do not split the reads.
// Everything in it is integer work or f64 additions in the host's order (flank_split of locus.hip, which the oracle pins), except two
// calls per read and candidate: exp and log, which are the device library's here and the platform libm's there.  The candidate search
// is therefore decided on the device only when it cannot depend on them:
//   every term is (mx + log(exp(t1 - mx) + exp(t2 - mx))) - ln2 with t1, t2, mx and the differences bit-identical on both sides (running
//   f64 sums of the same two constants in the same order; one of the differences is exactly 0 and its exp is taken as 1.0).  The other
//   argument d <= 0 gives exp(d) in (0, 1], the sum lies in [1, 2], its log L in [0, ln 2].  glibc documents at most 1 ulp for f64 exp
//   and log ("Known Maximum Errors in Math Functions" of its manual, every platform's column); the device library implements the
//   accuracy table of the OpenCL C specification (OpenCL 3.0 C, "Relative Error as ULPs", double precision: exp <= 3 ulp, log <= 3 ulp),
//   which the ROCm device-libs' OCML documentation names as its contract.  One ulp of a result <= 1 is at most 2^-52, of one below 1
//   2^-53.  So the two exps differ by at most 4 * 2^-52, the rounded sums by that and one ulp of [1, 2] more, the logs (slope <= 1) by
//   as much plus their own 4 * 2^-53: |L_host - L_device| < 2^-49.  mx + L and the subtraction of ln2 round once each, values of
//   magnitude <= |term| + 1.4 (every term is ln((e^t1 + e^t2) / 2) <= 0, so |M| is the sum of the |term|): at most 2^-51 * (|term| + 1.4)
//   between the two sides; the running sum over the reads rounds a partial sum <= |M| once per read on either side.  Over n <= 256
//   reads: n * 2^-49 + 2^-51 * (|M| + 1.4 n) + n * 2^-52 * |M| < 6.5e-13 * (1 + |M|) between the host's and the device's sum of one candidate.
// A locus is decided when the maximum M is ahead of every other candidate by more than delta = 2^-30 * (1 + |M|) -- 1 400 times that
// bound -- so that the host's search has the same single winner; otherwise it is handed to the host path (FL_UNDECIDED).  Margins
// of generated and hostile inputs, relative to 1 + |M|, are 0 (or a few 1e-15, where equal sums round apart) or >= 8e-4 (DESIGN.md
// section 2; tests/test_snv_split_cases.py holds its cases to <= 1e-12 or >= 1e-6).
// false: no split (FL_NOSPLIT: neither branch splits the reads, the host need not look) and the locus continues with the length
// genotype.  true: settled by flank_tail, or handed to the host path (sh.bail = 1).  Called by the whole wave with uniform arguments.
// The log-likelihood of one candidate genotype (h1, h2) over the kept reads in kept order (:171-204), by one thread: eval() of a read
// against either haplotype is a running sum over the ns SNVs ascending, the candidate's a running sum over the reads.  The expression
// order is flank_split's; prof(i, obs, val) loads the two masks of kept read i.  One function for the one-wave route below and the
// workgroup's (deep_snv_route of locus_gt_deep.hpp); a: the route's arguments with the three host-computed logarithms.
template <class A, class P>
__device__ __forceinline__ double snv_candidate_ll(const A& a, int n, int ns, uint64_t h1, uint64_t h2, P prof) {
  double ll = 0.0;
  for (int i = 0; i < n; ++i) {
    uint64_t obs, val;
    prof(i, obs, val);
    double t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < ns; ++k) {
      if (!((obs >> k) & 1ull)) continue;
      t1 += ((val ^ h1) >> k) & 1ull ? a.ln_mis : a.ln_match;
      t2 += ((val ^ h2) >> k) & 1ull ? a.ln_mis : a.ln_match;
    }
    const double mx = t1 > t2 ? t1 : t2;
    const double d1 = t1 - mx, d2 = t2 - mx;
    const double e1 = d1 == 0.0 ? 1.0 : exp(d1), e2 = d2 == 0.0 ? 1.0 : exp(d2);
    ll += (mx + log(e1 + e2)) - a.ln2;
  }
  return ll;
}

// The route is stated once, for the one-wave size genotyper and for the SNV forms behind the one-wave cluster chain
// (locus_cluster_flank.hpp).  sh: the route's LDS -- an SnvShared<MAXR, true> block beside the kept reads (s_read) and the assignment (cls);
// a: the route's arguments -- start_offset / end_offset (NULL = 0 for every read), mismatch_offsets / mismatch_off, and the three
// host-rounded logarithms ln_match, ln_mis, ln2.  END says how the route ends for its caller, and its results are snv_route's:
//   END::nosplit(sh, a, l, lane)       no split
//   END::handed(sh, a, l, lane, why)   beyond one of the three limits (why = 0) or not decided beyond the margin (FL_UNDECIDED)
//   END::split(sh, a, l, lane, cnt, hap)   the assignment is in sh.cls, sh.v_tie marks the reads that belong to both groups, cnt[g]
//                                      members and hap[g] assigned reads of either group (a group may be empty: no split)
// SizeEnd is the size genotyper's (the byte of the locus, sh.bail); its split is flank_tail, which stays where it was, inside snv_route
// (END::SIZE): the figures of the four SNV forms of locus_genotype_kernel move when it is called from anywhere else (two SGPR spills of
// one of them; profiles/snv_cluster_resource_usage.txt).  nu, fits, refn, refo are read by that tail only.
struct SizeEnd {
  static constexpr bool SIZE = true;
  template <class SH> static __device__ __forceinline__ bool nosplit(SH&, const SnvArgs& a, int64_t l, int lane) { if (lane == 0) a.flank_done[l] = FL_NOSPLIT | FL_SNV; return false; }
  template <class SH> static __device__ __forceinline__ bool handed(SH& sh, const SnvArgs& a, int64_t l, int lane, uint8_t why) { sh.bail = 1; if (lane == 0) a.flank_done[l] = FL_HANDED | FL_SNV | why; return true; }
};
template <int MAXR, class END = SizeEnd, class SH, class A>
__device__ __forceinline__ bool snv_route(SH& sh, const A& a, int64_t l, uint64_t r0, int n, int nu, int lane, bool fits, uint32_t refn, uint64_t refo) {
  constexpr int CAP = SNV_OFFS_PER_READ * MAXR;
  static_assert(CAP / 64 <= 32, "one bit per owned entry in `called`");
  auto nosplit = [&]() { return END::nosplit(sh, a, l, lane); };
  auto handed = [&](uint8_t why) { return END::handed(sh, a, l, lane, why); };
  // ---- get_analysis_region (:206-226): the skip-th largest start offset, the skip-th smallest end offset, by rank
  const int skip = (int)round((double)n * (1.0 - 0.85));
  if (skip >= n) return nosplit();
  for (int i = lane; i < n; i += 64) {
    const uint64_t r = r0 + sh.s_read[i];
    sh.v_so[i] = a.start_offset ? a.start_offset[r] : 0; sh.v_eo[i] = a.end_offset ? a.end_offset[r] : 0;
  }
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const int32_t s = sh.v_so[i], e = sh.v_eo[i];
    int rs = 0, re = 0;
    for (int j = 0; j < n; ++j) { const int32_t sj = sh.v_so[j], ej = sh.v_eo[j]; rs += sj < s || (sj == s && j < i); re += ej < e || (ej == e && j < i); }
    if (rs == n - 1 - skip) sh.v_reg[0] = s;
    if (re == skip) sh.v_reg[1] = e;
  }
  __syncthreads();
  const int32_t reg0 = sh.v_reg[0], reg1 = sh.v_reg[1];
  // ---- call_snvs (:271-286): the in-region offsets of all reads, 64 of one read's list per round, packed in read order
  int total = 0;
  for (int i = 0; i < n; ++i) {
    const uint64_t r = r0 + sh.s_read[i];
    const uint64_t m0 = a.mismatch_off[r], m1 = a.mismatch_off[r + 1];
    for (uint64_t base = m0; base < m1; base += 64) {
      const uint64_t k = base + (uint64_t)lane;
      const int32_t o = k < m1 ? a.mismatch_offsets[k] : 0;
      const bool in = k < m1 && reg0 <= o && o <= reg1;
      const unsigned long long bal = __ballot(in);
      const int at = total + __popcll(bal & ((1ull << lane) - 1ull));
      if (in && at < CAP) sh.v.offs[at] = o;
      total += __popcll(bal);
    }
  }
  __syncthreads();
  if (total == 0) return nosplit();  // no SNV: every profile is empty, one candidate genotype
  if (total > CAP) return handed(0);
  // an offset is called when its occurrences are at least 20 % of the reads; lane e owns entries e, e + 64, ...: the first occurrence speaks
  uint32_t called = 0;  // bit t: entry lane + 64 t is the first occurrence of a called offset
  for (int t = 0; t < CAP / 64; ++t) {
    const int e = lane + 64 * t;
    if (e >= total) break;
    const int32_t o = sh.v.offs[e];
    int c = 0; bool first = true;
    for (int j = 0; j < total; ++j) { const bool same = sh.v.offs[j] == o; c += same; first = first && !(same && j < e); }
    if (first && (double)c / (double)n >= 0.20) called |= 1u << t;
  }
  int ns = 0;
  for (int t = 0; t < CAP / 64; ++t) {
    if (64 * t >= total) break;
    const bool mine = (called >> t) & 1u;
    const unsigned long long bal = __ballot(mine);
    const int at = ns + __popcll(bal & ((1ull << lane) - 1ull));
    if (mine && at < SNV_MAX_SNVS) sh.v_tmp[at] = sh.v.offs[lane + 64 * t];
    ns += __popcll(bal);
  }
  __syncthreads();
  if (ns == 0) return nosplit();
  if (ns > SNV_MAX_SNVS) return handed(0);
  if (lane < ns) {  // ascending
    const int32_t o = sh.v_tmp[lane];
    int r = 0;
    for (int j = 0; j < ns; ++j) r += sh.v_tmp[j] < o;
    sh.v_snv[r] = o;
  }
  __syncthreads();  // (the offsets are done with: their bytes become the profiles)
  // ---- profiles (:250-269): SNV k of a read is None outside [start_offset, end_offset], else whether its list has the offset
  const uint64_t all = ns == 64 ? ~0ull : (1ull << ns) - 1ull;
  int full = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    uint64_t obs = 0, val = 0;
    if (i < n) {
      const uint64_t r = r0 + sh.s_read[i];
      const int32_t* m = a.mismatch_offsets + a.mismatch_off[r];
      const int nm = (int)(a.mismatch_off[r + 1] - a.mismatch_off[r]);
      const int32_t s = sh.v_so[i], e = sh.v_eo[i];
      for (int k = 0; k < ns; ++k) {
        const int32_t o = sh.v_snv[k];
        if (o < s || o > e) continue;
        obs |= 1ull << k;
        int lo = 0, hi = nm;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (m[mid] < o) lo = mid + 1; else hi = mid; }
        if (lo < nm && m[lo] == o) val |= 1ull << k;
      }
      sh.v.p.obs[i] = obs; sh.v.p.val[i] = val;
    }
    full += __popcll(__ballot(i < n && obs == all));
  }
  __syncthreads();
  // ---- candidate genotypes (:228-248): the distinct fully observed profiles in the derived order of Option<bool> -- first SNV most
  //      significant, false before true: the bit-reversed value mask -- and their pairs a <= b, a outer
  if ((double)full / (double)n < 0.40) return nosplit();
  int nh = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool first = i < n && sh.v.p.obs[i] == all;
    if (first) { const uint64_t v = sh.v.p.val[i]; for (int j = 0; j < i; ++j) first = first && !(sh.v.p.obs[j] == all && sh.v.p.val[j] == v); }
    if (i < n) sh.v_tie[i] = first ? 1 : 0;
    nh += __popcll(__ballot(first));
  }
  __syncthreads();
  if (nh * (nh + 1) / 2 <= 1) return nosplit();
  if (nh > SNV_MAX_HAPS) return handed(0);
  for (int i = lane; i < n; i += 64) {
    if (!sh.v_tie[i]) continue;
    const uint64_t key = __brevll(sh.v.p.val[i]);
    int r = 0;
    for (int j = 0; j < n; ++j) r += sh.v_tie[j] && __brevll(sh.v.p.val[j]) < key;
    sh.v_hap[r] = sh.v.p.val[i];
  }
  __syncthreads();
  // ---- log-likelihoods (:171-204), one lane per candidate, the reads in kept order; eval() is a running sum over the SNVs ascending
  const int nc = nh * (nh + 1) / 2;
  for (int c = lane; c < nc; c += 64) {
    int ha = 0, hb = 0;
    { int p = 0; for (int x = 0; x < nh; ++x) for (int y = x; y < nh; ++y, ++p) if (p == c) { ha = x; hb = y; } }
    sh.v_ll[c] = snv_candidate_ll(a, n, ns, sh.v_hap[ha], sh.v_hap[hb], [&](int i, uint64_t& obs, uint64_t& val) { obs = sh.v.p.obs[i]; val = sh.v.p.val[i]; });
  }
  __syncthreads();
  // ---- the decision: max_by's winner is the last maximum in candidate order; every other candidate must stay below M - delta
  double M = sh.v_ll[0]; int win = 0;
  for (int c = 1; c < nc; ++c) if (sh.v_ll[c] >= M) { M = sh.v_ll[c]; win = c; }
  const double delta = 0x1p-30 * (1.0 + fabs(M));
  bool decided = true;
  for (int c = 0; c < nc; ++c) if (c != win && sh.v_ll[c] >= M - delta) decided = false;
  if (!decided) return handed(FL_UNDECIDED);
  int wa = 0, wb = 0;
  { int p = 0; for (int x = 0; x < nh; ++x) for (int y = x; y < nh; ++y, ++p) if (p == win) { wa = x; wb = y; } }
  if (wa == wb) return nosplit();  // "homozygous"
  const uint64_t top1 = sh.v_hap[wa], top2 = sh.v_hap[wb];
  __syncthreads();  // (v_tie changes its meaning)
  // ---- the assignment (:114-137): fewer agreements with the first haplotype -> group 0, more -> group 1, as many -> both groups, and the
  //      assignment alternates from 0 (the k-th such read, k from 0, gets k % 2)
  int ties = 0, cnt[2] = {0, 0}, hap[2] = {0, 0};
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    int d1 = 0, d2 = 0;
    if (i < n) { const uint64_t obs = sh.v.p.obs[i], val = sh.v.p.val[i]; d1 = __popcll(obs & ~(val ^ top1)); d2 = __popcll(obs & ~(val ^ top2)); }
    const bool tie = i < n && d1 == d2;
    const unsigned long long tb = __ballot(tie);
    const int k = ties + __popcll(tb & ((1ull << lane) - 1ull));
    const int g = tie ? (k & 1) : (d1 < d2 ? 0 : 1);
    if (i < n) { sh.cls[i] = (int8_t)g; sh.v_tie[i] = tie ? 1 : 0; }
    const int here = n - base < 64 ? n - base : 64;
    const int ones = __popcll(__ballot(i < n && g == 1)), m1 = __popcll(__ballot(i < n && (g == 1 || tie))), m0 = __popcll(__ballot(i < n && (g == 0 || tie)));
    hap[1] += ones; hap[0] += here - ones; cnt[0] += m0; cnt[1] += m1;
    ties += __popcll(tb);
  }
  __syncthreads();
  if constexpr (END::SIZE) {
    if (!flank_tail<SnvMembers>(sh, a, l, n, nu, lane, fits, refn, refo, cnt, hap, (uint8_t)FL_SNV)) return nosplit();
    // a locus that waits for the repair chain leaves its split behind: flank_finish reads it and does not recompute it
    if (sh.bail == 2)
      for (int i = lane; i < n; i += 64)
        a.snv_read[r0 + i] = (uint8_t)((sh.cls[i] ? SR_ASSIGN : 0) | (SnvMembers::in(sh, i, 0) ? SR_IN0 : 0) | (SnvMembers::in(sh, i, 1) ? SR_IN1 : 0));
    return true;
  } else return END::split(sh, a, l, lane, cnt, hap);
}

// ---- the lane-parallel sections of locus_genotype_kernel.  Elements (kept reads, unique lengths, unique sequences) are spread over the
// wave as lane, lane + 64, ...: R = MAXR / 64 per lane.  Uniform arguments; every function is called by the whole wave.
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) { for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o); return v; }
__device__ __forceinline__ uint32_t wave_incl_sum_u(uint32_t v, int lane) {
  for (int o = 1; o < 64; o <<= 1) { const uint32_t w = (uint32_t)__shfl_up((int)v, o); if (lane >= o) v += w; }
  return v;
}
// how many loci of a call left the lane-parallel sections, and why (RC_GT_* of repair_queue.hpp; calls with the device-side repair)
__device__ __forceinline__ void gt_tally(const RepairBufs& rp, int word, int lane) { if (lane == 0 && rp.counts) atomicAdd(rp.counts + word, 1u); }

// LDS layout of the n repeat segments (4-aligned, in kept order) and of the reference repeat behind them: a prefix sum over the
// aligned lengths.  sh.fits = 0 when the sum passes SEG at any segment, or with the reference repeat behind the last one.
template <int MAXR, int SEG, class SH>
__device__ __forceinline__ void gt_layout(SH& sh, int n, uint32_t refn, int lane) {
  uint32_t carry = 0; bool over = false;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const uint32_t v = i < n ? (sh.s_len[i] + 3u) & ~3u : 0u;
    const uint32_t inc = wave_incl_sum_u(v, lane);
    if (i < n) sh.s_loff[i] = (uint16_t)(carry + inc - v);
    over = over || __ballot(i < n && carry + inc > (uint32_t)SEG) != 0ull;
    carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  }
  if (lane == 0) { sh.ref_off = carry; if (over || carry + ((refn + 3u) & ~3u) > (uint32_t)SEG) sh.fits = 0; }
}

// The segments of the n kept reads and, as item n, the reference repeat from global memory into their places in sh.bytes.  A group of
// 16 lanes takes K items at a time and has the first 256 bytes and the tail bytes of all K in flight before it stores any of them:
// the copy is bound by the latency of these loads, not by their number (longer items finish 256 bytes per round, as copy16 does).
template <int K, class SH>
__device__ __forceinline__ void gt_stage(SH& sh, const GtArgs& a, int n, uint32_t refn, uint64_t refo, int lane) {
  const int grp = lane >> 4, sub = lane & 15;
  for (int j0 = grp * K; j0 <= n; j0 += 4 * K) {
    const uint8_t* src[K]; uint8_t* dst[K]; uint32_t len[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = j0 + k;
      src[k] = a.tr_blob + refo; dst[k] = sh.bytes + sh.ref_off; len[k] = j == n ? refn : 0u;
      if (j < n) { src[k] = a.reads + sh.r_off[sh.s_read[j]] + sh.s_start[j]; dst[k] = sh.bytes + sh.s_loff[j]; len[k] = sh.s_len[j]; }
    }
    uint4 v[K]; uint8_t tl[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t full = len[k] >> 4, tb = full * 16 + (uint32_t)sub;
      if ((uint32_t)sub < full) __builtin_memcpy(&v[k], src[k] + 16 * sub, 16);
      if (tb < len[k]) tl[k] = src[k][tb];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t full = len[k] >> 4, tb = full * 16 + (uint32_t)sub;
      if ((uint32_t)sub < full) { uint32_t* d = reinterpret_cast<uint32_t*>(dst[k]) + 4 * sub; d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w; }
      if (tb < len[k]) dst[k][tb] = tl[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      for (uint32_t w = 16 + (uint32_t)sub; w < (len[k] >> 4); w += 16) {
        uint4 x; __builtin_memcpy(&x, src[k] + 16 * w, 16);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst[k]) + 4 * w;
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
      }
  }
}

// Unique lengths ascending with their multiplicities (sh.ulen, sh.ucnt, sh.n_sizes) of a kept list that is sorted by length: the runs.
// A lane per read marks where a run begins, the begins before it give the run its slot, the next begin its length.  false: the list
// is not sorted (the downsample moved reads) and the caller builds the histogram read by read.
template <int MAXR, class SH>
__device__ __forceinline__ bool gt_len_runs(SH& sh, int n, int lane) {
  int u = 0; bool sorted = true;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const uint32_t cur = i < n ? sh.s_len[i] : 0u, prev = i > 0 && i < n ? sh.s_len[i - 1] : 0u;
    sorted = sorted && __ballot(i > 0 && i < n && prev > cur) == 0ull;
    const bool begin = i < n && (i == 0 || prev != cur);
    const unsigned long long bb = __ballot(begin);
    if (begin) { const int s = u + __popcll(bb & ((1ull << lane) - 1ull)); sh.ulen[s] = cur; sh.ucnt[s] = (uint32_t)i; }
    u += __popcll(bb);
  }
  if (!sorted) return false;
  __syncthreads();
  uint32_t at[MAXR / 64], next[MAXR / 64];
#pragma unroll
  for (int t = 0; t < MAXR / 64; ++t) { const int s = lane + 64 * t; if (s < u) { at[t] = sh.ucnt[s]; next[t] = s + 1 < u ? sh.ucnt[s + 1] : (uint32_t)n; } }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < MAXR / 64; ++t) { const int s = lane + 64 * t; if (s < u) sh.ucnt[s] = next[t] - at[t]; }
  if (lane == 0) sh.n_sizes = u;
  return true;
}

// Which of the n kept reads carry the same sequence (segments staged in sh.bytes): fr[t] = the first kept read with the sequence of read
// lane + 64 t (-1 beyond n).  Every lane hashes its own segments (independent LDS loads), the first read of the same length and hash
// is found by passing the reads round the wave in kept order, and every read is then compared with that first read dword by dword
// (the tail mask of cmp_lds).  false: a comparison failed -- two sequences share length and hash -- and the caller takes every read
// singly.  weak: the hash is left out (developer switch: every pair of distinct sequences of one length collides).
template <int R, class SH>
__device__ __forceinline__ bool gt_equal_reads(SH& sh, int n, int lane, bool weak, int (&fr)[R]) {
  uint32_t ln[R], h1[R], h2[R];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const int i = lane + 64 * t;
    ln[t] = 0; h1[t] = 0x811C9DC5u; h2[t] = 0x9E3779B9u; fr[t] = -1;
    if (i >= n) continue;
    ln[t] = sh.s_len[i];
    if (weak) continue;
    const uint32_t* W = reinterpret_cast<const uint32_t*>(sh.bytes + sh.s_loff[i]);
    const uint32_t nw = (ln[t] + 3u) >> 2, tail = (ln[t] & 3u) ? (1u << (8 * (ln[t] & 3u))) - 1u : 0xFFFFFFFFu;
    for (uint32_t w = 0; w < nw; w += 4) {  // (words beyond the segment count as 0: the same for every segment of this length)
      uint32_t x[4];
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) { x[k] = w + k < nw ? W[w + k] : 0u; if (w + k == nw - 1) x[k] &= tail; }
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        h1[t] = (h1[t] ^ x[k]) * 0x9E3779B1u; h1[t] = (h1[t] << 13) | (h1[t] >> 19);
        h2[t] = (h2[t] + x[k]) * 0x85EBCA6Bu; h2[t] ^= h2[t] >> 15;
      }
    }
  }
#pragma unroll
  for (int tj = 0; tj < R; ++tj)
    for (int jl = 0; jl < 64 && 64 * tj + jl < n; ++jl) {
      const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)ln[tj], jl), a1 = (uint32_t)__builtin_amdgcn_readlane((int)h1[tj], jl),
                     a2 = (uint32_t)__builtin_amdgcn_readlane((int)h2[tj], jl);
#pragma unroll
      for (int t = 0; t < R; ++t)
        if (fr[t] < 0 && lane + 64 * t < n && ln[t] == lj && h1[t] == a1 && h2[t] == a2) fr[t] = 64 * tj + jl;
    }
  bool differ = false;
#pragma unroll
  for (int t = 0; t < R; ++t) {
    const int i = lane + 64 * t;
    if (i >= n || fr[t] == i) continue;
    const uint32_t* A = reinterpret_cast<const uint32_t*>(sh.bytes + sh.s_loff[i]);
    const uint32_t* B = reinterpret_cast<const uint32_t*>(sh.bytes + sh.s_loff[fr[t]]);
    const uint32_t nw = (ln[t] + 3u) >> 2, tail = (ln[t] & 3u) ? (1u << (8 * (ln[t] & 3u))) - 1u : 0xFFFFFFFFu;
    for (uint32_t w = 0; w < nw; w += 4) {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        if (w + k >= nw) break;
        uint32_t x = A[w + k] ^ B[w + k];
        if (w + k == nw - 1) x &= tail;
        differ = differ || x != 0u;
      }
    }
  }
  return __ballot(differ) == 0ull;
}

// make GTPROF=1 (developer build): lane 0 of every locus splits its shader-clock time over the sections of the kernel; the sums leave the
// kernel through a symbol of their own (locus.hip prints and clears it behind the launch of a TRGT_WFA_DEBUG call)
enum { GTP_FRONT = 0, GTP_STAGE, GTP_LENS, GTP_CAND, GTP_SEQ, GTP_ROUTE, GTP_PICK, GTP_CLASS, GTP_OUT, GTP_WORDS = 16 };
#ifdef TRGT_GT_PROF
__device__ unsigned long long g_gt_prof[GTP_WORDS];
#define GTP_DECL unsigned long long gtp_t = clock64()
#define GTP_MARK(i) do { const unsigned long long n_ = clock64(); if (threadIdx.x == 0) atomicAdd(&g_gt_prof[i], n_ - gtp_t); gtp_t = n_; } while (0)
#else
#define GTP_DECL
#define GTP_MARK(i)
#endif

template <int MAXR, int SEG, bool PRESEL = false, bool FLANK = false, bool SNV = false>
__global__ void __launch_bounds__(64) locus_genotype_kernel(const GtArgsOf<FLANK, SNV> a) {  // exactly one wave per locus: the lane-0 sections and the ballots rely on it
  static_assert(FLANK || !SNV, "the SNV forms are FLANK forms: they share the tail of the route and its LDS");
  __shared__ GtShared<MAXR, SEG, FLANK, SNV> sh;
  const int64_t l = blockIdx.x;
  if (l >= a.n_loci) return;
  const int lane = threadIdx.x;
  constexpr int R = MAXR / 64;  // elements per lane: lane owns lane, lane + 64, ...
  const bool serial = (a.finish_clears_need & GT_DEV_SERIAL) != 0, weak_hash = (a.finish_clears_need & GT_DEV_WEAK_HASH) != 0;
  const uint64_t r0 = a.locus_read_begin[l], r1 = a.locus_read_begin[l + 1];
  const int nr = (int)(r1 - r0);
  // (what the locus needs from global memory beside its reads, asked for here: each of these loads is a round trip of its own further down)
  const uint8_t ploidy_l = a.ploidy[l];
  const uint32_t refn = a.tr_len[l], allele_cap_l = a.allele_cap[l];
  const uint64_t refo = a.tr_off[l], allele_at[2] = {a.allele_off[2 * l], a.allele_off[2 * l + 1]};
  GTP_DECL;
  if (lane == 0) {
    sh.n = 0; sh.bail = 0; sh.fits = 1; sh.res_n_gt = 0;
    if (a.gt_size) a.gt_size[2 * l] = a.gt_size[2 * l + 1] = 0;
    if (a.skip_b) a.skip_b[l] = 1;
    a.need_host[l] = 0; a.n_alleles[l] = 0; a.n_spanning_reads[l] = 0; a.flipped[l] = 0;
    a.allele_len[2 * l] = a.allele_len[2 * l + 1] = 0; a.num_spanning[2 * l] = a.num_spanning[2 * l + 1] = 0;
    if constexpr (FLANK) a.flank_done[l] = 0;
  }
  const bool cluster = a.genotyper && a.genotyper[l] == 1;
  if (ploidy_l == 0 || nr == 0 || nr > MAXR || cluster) {  // Ploidy::Zero -> LocusResult::empty (tr.rs:29-31); oversized, cluster genotyper -> host
    for (int i = lane; i < nr; i += 64) { a.classification[r0 + i] = -1; a.read_rank[r0 + i] = -1; }
    if (lane == 0 && (nr > MAXR || cluster) && ploidy_l != 0 && nr != 0) a.need_host[l] = 1;
    return;
  }
  gt_selected<MAXR, PRESEL>(sh, a, l, r0, nr, lane);
  int n = sh.n;
  GTP_MARK(GTP_FRONT);
  if (n > 0) {
    // ---- LDS layout of the repeat segments (4-aligned) and of the reference repeat behind them
    //      (segments that do not fit are compared where they lie, in the read blob: sh.fits = 0)
    if (!serial) gt_layout<MAXR, SEG>(sh, n, refn, lane);
    else if (lane == 0) {
      uint32_t o = 0;
      for (int i = 0; i < n; ++i) { sh.s_loff[i] = (uint16_t)o; o += (sh.s_len[i] + 3u) & ~3u; if (o > (uint32_t)SEG) { sh.fits = 0; break; } }
      sh.ref_off = o;
      if (o + ((refn + 3u) & ~3u) > (uint32_t)SEG) sh.fits = 0;
    }
    __syncthreads();
    if (sh.fits) {
      if (!serial) gt_stage<4>(sh, a, n, refn, refo, lane);
      else {
        const int grp = lane >> 4, sub = lane & 15;
        for (int i = grp; i < n; i += 4) copy16(sh.bytes + sh.s_loff[i], a.reads + sh.r_off[sh.s_read[i]] + sh.s_start[i], sh.s_len[i], sub);
        if (grp == 0) copy16(sh.bytes + sh.ref_off, a.tr_blob + refo, refn, sub);
      }
    }
    __syncthreads();
  }
  const bool fits = sh.fits != 0;
  GTP_MARK(GTP_STAGE);
  auto seg_glob =[&](int i) { return a.reads + sh.r_off[sh.s_read[i]] + sh.s_start[i]; };
  auto cmp_seg = [&](int i, int j) {  // uniform arguments, uniform result
    return fits ? cmp_lds(sh.bytes + sh.s_loff[i], sh.s_len[i], sh.bytes + sh.s_loff[j], sh.s_len[j]) : cmp_bytes(seg_glob(i), sh.s_len[i], seg_glob(j), sh.s_len[j]);
  };
  if (n > 0 && !sh.bail) {
    // ---- unique lengths / counts ascending (sorted(lens) of genotype_size_front; after a downsample the list is not sorted)
    //      a sorted list -- every list that was not downsampled -- is cut into its runs by the whole wave
    const bool runs = !serial && gt_len_runs<MAXR>(sh, n, lane);
    if (!runs && !serial) gt_tally(a.rp, RC_GT_UNSORTED, lane);
    if (!runs && lane == 0) {  // (one lane builds the histogram: read-modify-writes of LDS by 64 lanes at once only work by lockstep)
      int u = 0;
      for (int i = 0; i < n; ++i) {
        const uint32_t v = sh.s_len[i];
        int p = 0;
        while (p < u && sh.ulen[p] < v) ++p;
        if (p < u && sh.ulen[p] == v) { sh.ucnt[p] += 1; continue; }
        for (int q = u; q > p; --q) { sh.ulen[q] = sh.ulen[q - 1]; sh.ucnt[q] = sh.ucnt[q - 1]; }
        sh.ulen[p] = v; sh.ucnt[p] = 1; ++u;
      }
      sh.n_sizes = u;
    }
    __syncthreads();
    const int u = sh.n_sizes;
    GTP_MARK(GTP_LENS);
    const int ploidy = ploidy_l == 1 ? 1 : 2;
    // ---- diploid::genotype / haploid::genotype: candidates spread over the lanes, first minimum wins
    double best_pen = 0.0; int best_p = 0x7FFFFFFF; bool have = false;
    if (ploidy == 2) {
      int p = 0;
      for (int si = 0; si < u; ++si)
        for (int li = si; li < u; ++li, ++p) {
          if ((p & 63) != lane) continue;
          const uint32_t sa = sh.ulen[si], la = sh.ulen[li];
          const double max_frac = adiff_u(sa, la) <= 100 ? 0.25 : 0.05;
          double pen = 0.0;
          for (int i = 0; i < u; ++i) {
            const uint32_t st = sh.ulen[i] != sa ? 10 + 2 * adiff_u(sa, sh.ulen[i]) : 0, lt = sh.ulen[i] != la ? 10 + 2 * adiff_u(la, sh.ulen[i]) : 0;
            const double term = (double)(st < lt ? st : lt) + max_frac * (double)(st > lt ? st : lt);
            pen += term * (double)sh.ucnt[i];
          }
          if (!have || pen < best_pen) { have = true; best_pen = pen; best_p = p; }
        }
    } else {
      for (int c = lane; c < u; c += 64) {
        double pen = 0.0;
        for (int i = 0; i < u; ++i) {
          const double term = sh.ulen[i] != sh.ulen[c] ? 10.0 + 2.0 * (double)adiff_u(sh.ulen[c], sh.ulen[i]) : 0.0;
          pen += term * (double)sh.ucnt[i];
        }
        if (!have || pen < best_pen) { have = true; best_pen = pen; best_p = c; }
      }
    }
    for (int o = 32; o > 0; o >>= 1) {  // (penalty, candidate index) minimum over the wave: the first minimum in candidate order
      const double op = __shfl_xor(best_pen, o); const int oi = __shfl_xor(best_p, o); const int oh = __shfl_xor((int)have, o);
      if (oh && (!have || op < best_pen || (op == best_pen && oi < best_p))) { have = true; best_pen = op; best_p = oi; }
    }
    GTP_MARK(GTP_CAND);
    // ---- the decisions are sequential and small: every lane takes them redundantly (uniform control flow, identical LDS
    //      writes), which lets the sequence comparisons use the whole wave
    {
      uint32_t size[2] = {0, 0}, civ[4] = {0, 0, 0, 0};
      int n_gt;
      if (ploidy == 2) {
        int si = 0, li = 0, p = 0;
        for (int x = 0; x < u; ++x) for (int y = x; y < u; ++y, ++p) if (p == best_p) { si = x; li = y; }
        const uint32_t bs = sh.ulen[si], bl = sh.ulen[li];
        uint32_t short_size = bs < bl ? bs : bl, long_size = bs > bl ? bs : bl;
        if (short_size != long_size && u >= 2) {
          uint64_t coverage = 0; int top = 0;
          for (int i = 0; i < u; ++i) { coverage += sh.ucnt[i]; if (sh.ucnt[i] > sh.ucnt[top]) top = i; }  // stable desc sort, first
          const double top_frac = (double)sh.ucnt[top] / (double)coverage;
          const uint32_t range = sh.ulen[u - 1] - sh.ulen[0];
          if (top_frac > 0.60 && range <= 6) short_size = long_size = sh.ulen[top];
        }
        n_gt = 2; size[0] = short_size; size[1] = long_size;
        civ[0] = civ[1] = short_size; civ[2] = civ[3] = long_size;
        for (int i = 0; i < u; ++i) {
          const uint32_t s = sh.ulen[i];
          if (adiff_u(s, short_size) <= adiff_u(s, long_size)) { civ[0] = civ[0] < s ? civ[0] : s; civ[1] = civ[1] > s ? civ[1] : s; }
          else { civ[2] = civ[2] < s ? civ[2] : s; civ[3] = civ[3] > s ? civ[3] : s; }
        }
      } else {
        n_gt = 1; size[0] = sh.ulen[best_p];
        civ[0] = sh.ulen[0]; civ[1] = sh.ulen[u - 1];
      }
      // ---- get_seq_hist: unique sequences in byte-lexicographic order (binary-search insertion into a sorted unique list)
      //      Which reads are equal is settled first, a lane per read (gt_equal_reads: fr[t] = the first kept read with the sequence of
      //      read lane + 64 t); the insertion then runs over those first reads only and adds each one's multiplicity.  Segments that are
      //      not staged, a hash collision and TRGT_GT_SERIAL leave every read its own first read, and the loop is the plain insertion of
      //      all n reads, which finds the equal ones itself (eq below).
      GTP_MARK(GTP_CAND);
      int fr[R];
      bool grouped = fits && !serial;
      if (grouped) { grouped = gt_equal_reads<R>(sh, n, lane, weak_hash, fr); if (!grouped) gt_tally(a.rp, RC_GT_COLLISION, lane); }
      else if (!serial) gt_tally(a.rp, RC_GT_NOFIT, lane);
      unsigned long long first[R];  // uniform: the reads to insert
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const int i = lane + 64 * t;
        if (!grouped) fr[t] = i < n ? i : -1;
        first[t] = __ballot(i < n && fr[t] == i);
        if constexpr (FLANK) { if (i < n) sh.f_uidx[i] = (uint16_t)fr[t]; }
      }
      __syncthreads();
      int nu = 0;
#pragma unroll
      for (int t = 0; t < R; ++t) {
        for (unsigned long long m = first[t]; m; m &= m - 1ull) {
          const int i = 64 * t + __ffsll((long long)m) - 1;
          int mult = 0;
#pragma unroll
          for (int tt = 0; tt < R; ++tt) mult += __popcll(__ballot(fr[tt] == i));
          int lo = 0, hi = nu, eq = -1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int r = sh.u_rep[mid];
            const int c = cmp_seg(i, r);
            if (c == 0) { eq = mid; break; }
            if (c < 0) hi = mid; else lo = mid + 1;
          }
          // (the list is written by lane 0 only; the comparisons of the next round read it back in program order: one wave, one LDS queue)
          if (eq >= 0) { if (lane == 0) { sh.u_cnt[eq] += (uint16_t)mult; if constexpr (FLANK) sh.f_uidx[i] = sh.u_rep[eq]; } continue; }
          if (lane == 0) {
            for (int q = nu; q > lo; --q) { sh.u_rep[q] = sh.u_rep[q - 1]; sh.u_cnt[q] = sh.u_cnt[q - 1]; }
            sh.u_rep[lo] = (uint16_t)i; sh.u_cnt[lo] = (uint16_t)mult;
          }
          ++nu;
        }
      }
      __syncthreads();
      GTP_MARK(GTP_SEQ);
      // ---- FLANK: two sizes at most 10 apart (tr.rs:69-75) and tags that split the reads replace everything below; the size
      //      genotyper's own repair is not queued for such a locus
      bool by_tags = false;
      if constexpr (SNV) {
        // ---- SNV: in the reference's order -- tags that split the reads own the locus (flank_route with both settings on; else the host
        //      finds the split as before: the byte stays 0), and only without such tags the SNVs of the flanks are tried
        if (n_gt == 2 && adiff_u(size[0], size[1]) <= 10) {
          int cnt[2];
          if (a.hp_tag && flank_assign(sh, a.hp_tag, r0, n, lane, cnt)) by_tags = a.tag_route && flank_tail<TagMembers>(sh, a, l, n, nu, lane, fits, refn, refo, cnt, cnt, (uint8_t)0);
          else by_tags = snv_route<MAXR>(sh, a, l, r0, n, nu, lane, fits, refn, refo);
        }
      } else if constexpr (FLANK) {
        if (a.hp_tag && n_gt == 2 && adiff_u(size[0], size[1]) <= 10) by_tags = flank_route(sh, a, l, r0, n, nu, lane, fits, refn, refo);
      }
      auto ulen_of = [&](int q) { return sh.s_len[sh.u_rep[q]]; };
      GTP_MARK(GTP_ROUTE);
      // ---- the picks: lane q holds the length and the multiplicity of unique sequence q (q + 64 t), the loops over the list are
      //      ballots and reductions.  closest: the first minimum in u_rep order; most_frequent: the last maximum (>=).
      uint32_t ql[R], qc[R];
#pragma unroll
      for (int t = 0; t < R; ++t) { const int q = lane + 64 * t; ql[t] = q < nu ? ulen_of(q) : 0u; qc[t] = q < nu ? sh.u_cnt[q] : 0u; }
      auto len_in_group = [&](uint32_t len, int al) {
        if (n_gt == 1) return true;
        const uint32_t d1 = adiff_u(len, size[0]), d2 = adiff_u(len, size[1]);
        return al == 0 ? d1 <= d2 : d2 < d1;
      };
      auto in_group = [&](int q, int al) { return len_in_group(ulen_of(q), al); };
      auto closest = [&](uint32_t target) {
        if (serial) { uint32_t c = ulen_of(0); for (int q = 0; q < nu; ++q) if (adiff_u(c, target) > adiff_u(ulen_of(q), target)) c = ulen_of(q); return c; }
        uint32_t d[R], best = 0xFFFFFFFFu;
#pragma unroll
        for (int t = 0; t < R; ++t) { d[t] = lane + 64 * t < nu ? adiff_u(ql[t], target) : 0xFFFFFFFFu; best = d[t] < best ? d[t] : best; }
        best = wave_min_u(best);
        uint32_t c = 0;
#pragma unroll
        for (int t = R - 1; t >= 0; --t) {
          const unsigned long long bal = __ballot(lane + 64 * t < nu && d[t] == best);
          if (bal) c = (uint32_t)__builtin_amdgcn_readlane((int)ql[t], __ffsll((long long)bal) - 1);
        }
        return c;
      };
      auto most_frequent = [&](uint32_t len) {
        if (serial) { int best = -1; for (int q = 0; q < nu; ++q) if (ulen_of(q) == len && (best < 0 || sh.u_cnt[q] >= sh.u_cnt[best])) best = q; return best; }
        uint32_t mx = 0;
#pragma unroll
        for (int t = 0; t < R; ++t) if (lane + 64 * t < nu && ql[t] == len && qc[t] > mx) mx = qc[t];
        mx = wave_max_u(mx);
        int best = -1;
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const unsigned long long bal = __ballot(lane + 64 * t < nu && ql[t] == len && qc[t] == mx);
          if (bal) best = 64 * t + 63 - __clzll((long long)bal);
        }
        return best;
      };
      int pick[2] = {most_frequent(closest(size[0])), -1};
      int n_pick = 1;
      if (n_gt != 1 && size[0] != size[1]) { pick[1] = most_frequent(closest(size[1])); n_pick = 2; }
      bool majority = true, lacks[2] = {false, false};
      for (int al = 0; al < n_pick; ++al) {  // split(): majority support of the pick inside its group, else stage B is needed
        uint64_t coverage = 0, ref_count = 0;
        if (serial) {
          for (int q = 0; q < nu; ++q) {
            if (!in_group(q, al)) continue;
            coverage += sh.u_cnt[q];
            if (q == pick[al]) ref_count = sh.u_cnt[q];
          }
        } else {
          uint32_t cov = 0, ref = 0;
#pragma unroll
          for (int t = 0; t < R; ++t) {
            const int q = lane + 64 * t;
            if (q < nu && len_in_group(ql[t], al)) { cov += qc[t]; if (q == pick[al]) ref = qc[t]; }
          }
          coverage = wave_sum_u(cov); ref_count = wave_sum_u(ref);
        }
        if (!(2 * ref_count >= coverage)) { majority = false; lacks[al] = true; }
      }
      GTP_MARK(GTP_PICK);
      if (by_tags) {}
      else if (!majority) {
        // ---- stage B on the device: one vote group per allele without majority support, one alignment job per unique sequence of
        //      its group against the pick (the members of make_consensus, genotype_size.rs:32-37), all segments of the read blob
        const RepairBufs& rp = a.rp;
        bool can = rp.counts != nullptr;
        uint32_t nm[2] = {0, 0}; unsigned long long mbytes[2] = {0, 0};
        if (can)
          for (int al = 0; al < n_pick; ++al) {
            if (!lacks[al]) continue;
            if (ulen_of(pick[al]) > rp.max_seg) can = false;
            for (int q = 0; q < nu; ++q) {
              if (!in_group(q, al)) continue;
              if (ulen_of(q) > rp.max_seg) can = false;
              nm[al] += 1; mbytes[al] += ulen_of(q);
            }
          }
        GroupNeeds nd[2] = {};
        if (can) {
#pragma unroll
          for (int al = 0; al < 2; ++al) if (lacks[al]) nd[al] = group_needs(ulen_of(pick[al]), nm[al], mbytes[al], rp.vote_lds_pos);
          if (lane == 0) repair_reserve(rp, l, a.n_loci, nm[0] + nm[1], (uint32_t)lacks[0] + (uint32_t)lacks[1], nd, sh.rsv);
          __syncthreads();
          can = sh.rsv.ok != 0;
        }
        if (!can) sh.bail = 1;
        else {
          Reserved at = sh.rsv;
          auto seg_of = [&](int q) { const int r = sh.u_rep[q]; return Seg{sh.r_off[sh.s_read[r]] + sh.s_start[r], sh.s_len[r]}; };  // of a unique sequence
          RepairPend pd;
          pd.n_gt = n_gt; pd.n_pick = n_pick; pd.size[0] = size[0]; pd.size[1] = size[1];
          for (int k = 0; k < 4; ++k) pd.civ[k] = (int32_t)civ[k];
          pd.rep[0] = pd.rep[1] = -1; pd.grp[0] = pd.grp[1] = -1;
#pragma unroll
          for (int al = 0; al < 2; ++al) {
            if (al >= n_pick) break;
            pd.rep[al] = sh.u_rep[pick[al]];
            if (lacks[al]) pd.grp[al] = (int32_t)queue_group<64>(rp.groups, rp.jobs, at, seg_of(pick[al]), nm[al], nd[al], nu, [&, al](int q) { return in_group(q, al); }, seg_of);
          }
          if (lane == 0) rp.pend[l] = pd;
          sh.bail = 2;  // the locus waits for repair_finish_kernel
        }
      }
      else {
        // ---- classification (genotype_size.rs:42-61), reference allele first (tr.rs:95-101)
        int rep[2]; uint32_t aln[2];
        for (int al = 0; al < n_pick; ++al) { rep[al] = sh.u_rep[pick[al]]; aln[al] = sh.s_len[rep[al]]; }
        int n_al = n_pick;
        if (ploidy == 2 && n_al == 1) { rep[1] = rep[0]; aln[1] = aln[0]; n_al = 2; }
        int by_hap[2] = {0, 0};
        if (serial) {
          int tie = 1;
          for (int i = 0; i < n; ++i) {
            int cc = 0;
            if (n_al == 2) {
              const uint32_t d1 = adiff_u(sh.s_len[i], aln[0]), d2 = adiff_u(sh.s_len[i], aln[1]);
              if (d1 < d2) cc = 0; else if (d1 > d2) cc = 1; else { tie = (tie + 1) % 2; cc = tie; }
            }
            sh.cls[i] = (int8_t)cc; by_hap[cc] += 1;
          }
        } else {
          // a lane per read; the k-th tied read, k from 0, gets k % 2 (the tie toggle starts at 1 and is advanced before use)
          int ties = 0;
          for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int cc = 0; bool tied = false;
            if (n_al == 2 && i < n) {
              const uint32_t d1 = adiff_u(sh.s_len[i], aln[0]), d2 = adiff_u(sh.s_len[i], aln[1]);
              cc = d1 > d2 ? 1 : 0; tied = d1 == d2;
            }
            const unsigned long long tb = __ballot(tied);
            if (tied) cc = (ties + __popcll(tb & ((1ull << lane) - 1ull))) & 1;
            if (i < n) sh.cls[i] = (int8_t)cc;
            const int ones = __popcll(__ballot(i < n && cc == 1));
            by_hap[1] += ones; by_hap[0] += (n - base < 64 ? n - base : 64) - ones;
            ties += __popcll(tb);
          }
        }
        auto eq_ref = [&](int al) {
          return fits ? cmp_lds(sh.bytes + sh.s_loff[rep[al]], aln[al], sh.bytes + sh.ref_off, refn) == 0 : cmp_bytes(seg_glob(rep[al]), aln[al], a.tr_blob + refo, refn) == 0;
        };
        int order[2] = {0, 1}; int flip = 0;
        if (n_gt != 1 && !eq_ref(0) && eq_ref(1)) { order[0] = 1; order[1] = 0; flip = 1; }
        for (int oi = 0; oi < n_gt; ++oi)
          if (aln[order[oi]] > allele_cap_l) sh.bail = 1;  // the host path reports the error
        sh.res_n_gt = n_gt; sh.res_flip = flip;
        for (int oi = 0; oi < n_gt; ++oi) {
          const int al = order[oi];
          sh.res_rep[oi] = rep[al]; sh.res_ci[2 * oi] = (int)civ[2 * al]; sh.res_ci[2 * oi + 1] = (int)civ[2 * al + 1]; sh.res_hap[oi] = by_hap[al];
        }
      }
    }
    __syncthreads();
    GTP_MARK(GTP_CLASS);
  }
  // ---- outputs, by the whole wave
  const bool done = n > 0 && !sh.bail;
  if (serial) {
    for (int i = lane; i < nr; i += 64) { a.classification[r0 + i] = -1; a.read_rank[r0 + i] = -1; }
    if (n > 0 && sh.bail) { if (lane == 0) a.need_host[l] = (uint8_t)(sh.bail == 2 ? 2 : 1); return; }
    if (!done) return;
    __syncthreads();  // the -1 defaults above are ordered before the entries of the kept reads (same wave, same addresses)
  } else {
    // every read's entries are written once: its rank among the kept reads (-1: not kept, or no genotype) is collected in LDS first
    // (r_len is done with behind the selection), so that no store waits for an earlier one to the same address
    int32_t* rank = reinterpret_cast<int32_t*>(sh.r_len);
    for (int i = lane; i < nr; i += 64) rank[i] = -1;
    __syncthreads();
    if (done) for (int i = lane; i < n; i += 64) if (sh.s_read[i] < (uint32_t)nr) rank[sh.s_read[i]] = i;
    __syncthreads();
    const int flip_all = done ? sh.res_flip : 0;
    for (int i = lane; i < nr; i += 64) {
      const int rk = rank[i];
      a.classification[r0 + i] = rk < 0 ? -1 : (flip_all ? 1 - sh.cls[rk] : sh.cls[rk]);
      a.read_rank[r0 + i] = rk;
    }
    if (n > 0 && sh.bail) { if (lane == 0) a.need_host[l] = (uint8_t)(sh.bail == 2 ? 2 : 1); return; }
    if (!done) return;
  }
  const int n_gt = sh.res_n_gt;
  for (int oi = 0; oi < n_gt; ++oi) {
    const int rep = sh.res_rep[oi];
    const uint32_t len = sh.s_len[rep];
    const uint8_t* src = fits ? sh.bytes + sh.s_loff[rep] : seg_glob(rep);
    uint8_t* dst = a.allele_blob + allele_at[oi];
    for (uint32_t b = lane; b < len; b += 64) dst[b] = src[b];
    if (lane == 0) {
      a.allele_len[2 * l + oi] = len;
      a.ci[4 * l + 2 * oi] = sh.res_ci[2 * oi]; a.ci[4 * l + 2 * oi + 1] = sh.res_ci[2 * oi + 1];
      a.num_spanning[2 * l + oi] = sh.res_hap[oi];
      if (a.gt_size) a.gt_size[2 * l + oi] = (int32_t)len;  // (a pick with majority support has the genotype's size)
    }
  }
  if (serial)
    for (int i = lane; i < n; i += 64) {
      a.classification[r0 + sh.s_read[i]] = sh.res_flip ? 1 - sh.cls[i] : sh.cls[i];
      a.read_rank[r0 + sh.s_read[i]] = i;
    }
  if (lane == 0) { a.n_alleles[l] = n_gt; a.n_spanning_reads[l] = (uint32_t)n; a.flipped[l] = (uint8_t)sh.res_flip; }
  GTP_MARK(GTP_OUT);
}

// ---- behind the consensus alignments and the column voting of the loci that waited for a repair: the rest of genotype_size::genotype
// (classification of the reads against the repaired alleles, genotype_size.rs:42-61), reference allele first (tr.rs:95-101), outputs.
// One wave per waiting locus (list in rp.loci).  A locus whose repaired allele does not fit (vote overflow, allele_cap) goes to the
// host path after all (need_host = 1); the others leave with need_host = 0.
template <int MAXR>
struct FinShared {
  uint32_t r_s[MAXR], r_len[MAXR]; uint64_t r_off[MAXR];
  uint32_t s_read[MAXR], s_start[MAXR], s_len[MAXR];
  int8_t cls[MAXR];
  int n;
};
// equality of two byte strings in global memory, by the whole wave (uniform arguments, uniform result)
__device__ __forceinline__ bool wave_equal(const uint8_t* __restrict__ p, uint32_t n, const uint8_t* __restrict__ q, uint32_t m) {
  if (n != m) return false;
  bool diff = false;
  for (uint32_t i = threadIdx.x & 63; i < n; i += 64) diff = diff || p[i] != q[i];
  return __ballot(diff) == 0ull;
}
// ... and of a locus the haplotype-tag route left waiting (RP_FLANK): the assignment is recomputed from the tags (deterministic from the
// same list of kept reads), the alleles are the repaired sequences or the backbones; smaller allele first (genotype_flank.rs:33-38), the
// assignment is the classification, its counts are num_spanning, the sizes of the genotype are the allele lengths
// (snv: the record is the SNV branch's -- its assignment is read back from SnvArgs::snv_read, SR_ASSIGN of every kept read, instead)
template <class SH>
__device__ __forceinline__ void flank_finish(SH& sh, const GtFlankArgs& a, const FinishArgs& f, const RepairPend& pd, int64_t l, uint64_t r0, int n, int lane,
                                             const uint8_t* __restrict__ snv = nullptr) {
  const RepairBufs& rp = a.rp;
  int cnt[2] = {0, 0};
  const uint8_t mark = snv ? (uint8_t)FL_SNV : (uint8_t)0;
  bool fail;
  if (snv) {
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const int g = i < n ? snv[r0 + i] & SR_ASSIGN : 0;
      if (i < n) sh.cls[i] = (int8_t)g;
      const int ones = __popcll(__ballot(i < n && g == 1));
      cnt[1] += ones; cnt[0] += (n - base < 64 ? n - base : 64) - ones;
    }
    __syncthreads();
    fail = n == 0;
  } else fail = n == 0 || !flank_assign(sh, a.hp_tag, r0, n, lane, cnt);
  const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0};
  auto seg_of = [&](int i) { return Seg{sh.r_off[sh.s_read[i]] + sh.s_start[i], sh.s_len[i]}; };
  for (int g = 0; g < 2 && !fail; ++g) fail = !repaired_allele(pd, g, f, rp, a.reads, seg_of, ap[g], aln[g]);
  const int sw = aln[0] > aln[1] ? 1 : 0;
  int order[2] = {sw, 1 - sw}, flip = 0;  // output allele -> tag group
  if (!fail) {
    const uint8_t* ref = a.tr_blob + a.tr_off[l]; const uint32_t refn = a.tr_len[l];
    if (!wave_equal(ap[order[0]], aln[order[0]], ref, refn) && wave_equal(ap[order[1]], aln[order[1]], ref, refn)) { order[0] = 1 - sw; order[1] = sw; flip = 1; }
    if (aln[0] > a.allele_cap[l] || aln[1] > a.allele_cap[l]) fail = true;  // the host path reports the error
  }
  if (fail) { if (lane == 0) { a.need_host[l] = 1; a.flank_done[l] = FL_HANDED | mark; } return; }
  for (int oi = 0; oi < 2; ++oi) {
    const int g = order[oi];
    uint8_t* dst = a.allele_blob + a.allele_off[2 * l + oi];
    for (uint32_t b = lane; b < aln[g]; b += 64) dst[b] = ap[g][b];
    if (lane == 0) {
      a.allele_len[2 * l + oi] = aln[g];
      a.ci[4 * l + 2 * oi] = pd.civ[2 * g]; a.ci[4 * l + 2 * oi + 1] = pd.civ[2 * g + 1];
      a.num_spanning[2 * l + oi] = cnt[g];
      if (a.gt_size) a.gt_size[2 * l + oi] = (int32_t)aln[g];
    }
  }
  for (int i = lane; i < n; i += 64) {
    a.classification[r0 + sh.s_read[i]] = sh.cls[i] == order[0] ? 0 : 1;
    a.read_rank[r0 + sh.s_read[i]] = i;
  }
  if (lane == 0) {
    a.n_alleles[l] = 2; a.n_spanning_reads[l] = (uint32_t)n; a.flipped[l] = (uint8_t)flip; a.skip_b[l] = 0; if (a.finish_clears_need) a.need_host[l] = 0;
    a.flank_done[l] = FL_DONE | FL_REPAIRED | mark;
  }
}
template <int MAXR, bool PRESEL = false, bool FLANK = false, bool SNV = false>
__global__ void __launch_bounds__(64) repair_finish_kernel(const GtArgsOf<FLANK, SNV> a, const FinishArgs f) {
  __shared__ FinShared<MAXR> sh;
  const RepairBufs& rp = a.rp;
  if (blockIdx.x >= rp.counts[RC_LOCI]) return;
  const int64_t l = rp.loci[blockIdx.x];
  const int lane = threadIdx.x;
  const uint64_t r0 = a.locus_read_begin[l];
  const int nr = (int)(a.locus_read_begin[l + 1] - r0);
  if (nr > MAXR) return;  // a locus of the deep size list (locus_gt_deep.hpp): deep_size_finish_kernel's
  if (lane == 0) sh.n = 0;
  gt_selected<MAXR, PRESEL>(sh, a, l, r0, nr, lane);
  const int n = sh.n;
  const RepairPend pd = rp.pend[l];
  if constexpr (FLANK) {
    if constexpr (SNV) {
      if (pd.n_pick & RP_SNV) { flank_finish(sh, a, f, pd, l, r0, n, lane, a.snv_read); return; }
    }
    if (pd.n_pick & RP_FLANK) { flank_finish(sh, a, f, pd, l, r0, n, lane); return; }
  }
  const int ploidy = a.ploidy[l] == 1 ? 1 : 2;
  // the alleles: the repaired sequence of a group, or the pick that had majority support
  const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0};
  bool fail = n == 0;
  auto seg_of = [&](int i) { return Seg{sh.r_off[sh.s_read[i]] + sh.s_start[i], sh.s_len[i]}; };
  for (int al = 0; al < pd.n_pick && !fail; ++al) fail = !repaired_allele(pd, al, f, rp, a.reads, seg_of, ap[al], aln[al]);
  int n_al = pd.n_pick;
  if (!fail && ploidy == 2 && n_al == 1) { ap[1] = ap[0]; aln[1] = aln[0]; n_al = 2; }
  int by_hap[2] = {0, 0}, order[2] = {0, 1}, flip = 0;
  if (!fail) {
    int tie = 1;  // (every lane walks the reads: uniform, and the list is short)
    for (int i = 0; i < n; ++i) {
      int cc = 0;
      if (n_al == 2) {
        const uint32_t d1 = adiff_u(sh.s_len[i], aln[0]), d2 = adiff_u(sh.s_len[i], aln[1]);
        if (d1 < d2) cc = 0; else if (d1 > d2) cc = 1; else { tie = (tie + 1) % 2; cc = tie; }
      }
      if (lane == 0) sh.cls[i] = (int8_t)cc;
      by_hap[cc] += 1;
    }
    const uint8_t* ref = a.tr_blob + a.tr_off[l]; const uint32_t refn = a.tr_len[l];
    if (pd.n_gt != 1 && !wave_equal(ap[0], aln[0], ref, refn) && wave_equal(ap[1], aln[1], ref, refn)) { order[0] = 1; order[1] = 0; flip = 1; }
    for (int oi = 0; oi < pd.n_gt; ++oi) if (aln[order[oi]] > a.allele_cap[l]) fail = true;  // the host path reports the error
  }
  __syncthreads();
  if (fail) { if (lane == 0) a.need_host[l] = 1; return; }
  for (int oi = 0; oi < pd.n_gt; ++oi) {
    const int al = order[oi];
    uint8_t* dst = a.allele_blob + a.allele_off[2 * l + oi];
    for (uint32_t b = lane; b < aln[al]; b += 64) dst[b] = ap[al][b];
    if (lane == 0) {
      a.allele_len[2 * l + oi] = aln[al];
      a.ci[4 * l + 2 * oi] = pd.civ[2 * al]; a.ci[4 * l + 2 * oi + 1] = pd.civ[2 * al + 1];
      a.num_spanning[2 * l + oi] = by_hap[al];
      if (a.gt_size) a.gt_size[2 * l + oi] = (int32_t)pd.size[al];
    }
  }
  for (int i = lane; i < n; i += 64) {
    a.classification[r0 + sh.s_read[i]] = flip ? 1 - sh.cls[i] : sh.cls[i];
    a.read_rank[r0 + sh.s_read[i]] = i;
  }
  // (need_host stays 2: the HMM batch of the loci settled by the genotyper may be reading it right now; the host turns 2 into skip_b)
  if (lane == 0) { a.n_alleles[l] = pd.n_gt; a.n_spanning_reads[l] = (uint32_t)n; a.flipped[l] = (uint8_t)flip; a.skip_b[l] = 0; if (a.finish_clears_need) a.need_host[l] = 0; }
}

}  // namespace gt
}  // namespace trgt
