// trgt_amd/csrc/locus_cluster_flank_deep.hpp -- the haplotype-tag branch of genotype_flank::genotype (genotype_flank.rs:9-76, 147-170;
// applied by analyze at tr.rs:64-75) for Genotyper::Cluster loci of more than gt::GT_MAX_READS candidate reads, behind the deep cluster
// chain of locus_cluster_deep.hpp: what locus_cluster_flank.hpp does for one wave, restated for one WORKGROUP of cld::DW threads per locus
// of the deep list.  On a context that opted in (trgt_hip_set_flank_cluster_deep_device, a setting of its own) and also has a deep cluster
// chain (trgt_hip_set_cluster_max_reads), for a batch with haplotype tags, two kernels follow cld::deep_finish_kernel:
//   deep_cluster_flank_kernel          a locus the chain completed with two alleles at most 10 apart: assignment by tag
//                                      (gtd::deep_flank_assign, the deep size route's), simple_consensus of either group; without a group
//                                      below 50 % the locus is settled here, else the groups are queued (repair_queue.hpp) for a THIRD
//                                      consensus round of the deep list -- BiWFA + consensus_vote_kernel over the third part of its job and
//                                      group lists -- and the locus waits (flank_done = FL_REPAIRED)
//   deep_cluster_flank_finish_kernel   the waiting loci: alleles = voted consensus or backbone, same order and outputs
// The kept reads are the deep chain's global lists (DeepArgs::sel_read / sel_start / sel_len at locus_read_begin + rank, ClRec::n of them).
// The cluster chain has no sequence histogram, so equal segments are found where they lie in the read blob -- up to 2 048^2 / 2 pairs:
// every thread reads the segments of its reads ONCE and leaves (length, 64-bit hash) in LDS; the all-pairs pass then runs on LDS alone and
// compares bytes in HBM only where length and hash agree, which keeps the comparison exact whatever the hash does.  Ties as in
// locus_cluster_deep.hpp: every choice is a minimum over values that do not depend on the thread that looked at them.
// A locus whose tags do not split its reads is not touched (the byte stays 0: the host sees it as before and tries the SNV branch); one that
// finds no room in the arenas, whose vote overflows or whose allele exceeds allele_cap is handed back (need_host = 1, FL_HANDED) and takes
// the host path.  The kernels of locus_cluster_deep.hpp and locus_cluster_flank.hpp are used as they are.
// The SNV forms of the two kernels (contexts that opted in with trgt_hip_set_snv_cluster_deep_device, batches that carry mismatch offsets)
// add the other branch, get_trs_with_clustering (genotype_flank.rs:78-138, 171-290), in the reference's order: tags that split the reads
// own the locus (this route with both settings on, else the host as before: the byte stays 0), and only without such tags the search of
// gtd::deep_snv_search runs -- the one of the deep size route, with its limits and its margin rule (locus_gt_deep.hpp).  Its groups
// overlap as behind the one-wave chain (locus_cluster_flank.hpp): a read that agrees equally with both haplotypes is a member of both
// while its assignment alternates; multiplicities, medians, the 50 % test, intervals and the third round's members follow the membership,
// num_spanning and the classification the assignment.  The bytes carry FL_SNV: FL_NOSPLIT (the host need not look again), FL_DONE, or
// FL_HANDED (limits, FL_UNDECIDED, and the hand-backs of the tag route).
#pragma once
#include "locus_cluster_flank.hpp"
#include "locus_gt_deep.hpp"

namespace trgt {
namespace cldf {

using cld::DT; using cld::DW; using cld::Red;
constexpr int MAXR = cld::CL_DEEP_MAX_READS;

// the deep route's own count block, laid out like clf::CF_* (the arenas are the deep chain's: CC_CIGAR / CC_OUT / CC_SCRATCH of its block)
enum { DF_J3 = 0 /* jobs of the third round */, DF_G3 = 1 /* vote groups */, DF_FAILED = 2 /* loci handed back */, DF_WORDS = 16 };
static_assert((int)DF_J3 == (int)clf::CF_J3 && (int)DF_G3 == (int)clf::CF_G3 && (int)DF_FAILED == (int)clf::CF_FAILED && (int)DF_WORDS == (int)clf::CF_WORDS, "laid out like CF_*");

// DeepArgs is the argument of every deep kernel and does not grow: what the two kernels read beyond it
struct DeepClFlankArgs {
  cld::DeepArgs d;
  const int16_t* hp_tag;   // per read of the batch: the HP tag (-1 = None)
  uint8_t* flank_done;     // [n_loci] gt::FL_*, written for the loci of the deep list only
  uint32_t* fcounts;       // [DF_WORDS]
  clf::ClFlankPend* pend;  // [n_list]
  uint32_t first_job, first_group;  // the third part of the deep list's job and group lists
};

// ... and what the SNV forms read beyond that (a struct of its own: DeepClFlankArgs does not grow): what clf::ClSnvArgs adds to
// clf::ClFlankArgs, and the workspace of the deep search in HBM -- the one of the deep size list's SNV forms.  Both deep lists can share
// prof, stage and snv_read in one call: they are indexed by read slot of the batch, the loci of the two lists are disjoint, and the
// chains run on one stream.
struct DeepClSnvArgs : DeepClFlankArgs {
  const int32_t *start_offset, *end_offset;  // per read of the batch (NULL = 0 for every read, as in flank_split)
  const int32_t* mismatch_offsets; const uint64_t* mismatch_off;  // per read r: its ascending offsets in [mismatch_off[r], mismatch_off[r + 1])
  uint8_t* snv_read;      // per read slot of the batch, by position in the kept list: gt::SR_* of a locus the search split
  int32_t* pend_hap;      // [2 n_list] beside pend: the assigned reads of either group (ClFlankPend::cnt holds the members)
  double ln_match, ln_mis, ln2;  // ln 0.9, ln(1.0 - 0.9), ln 2 as the host's libm rounds them
  int32_t tag_route;      // 1: tags that split the reads are this route's (trgt_hip_set_flank_cluster_deep_device is on as well); 0: the host's
  uint64_t* prof;         // [2 x read slots of the batch] kept read i of a locus: its observed mask at 2 (r0 + i), its value mask behind it
  int32_t* stage;         // [stage_cap = mismatch_off[reads of the batch]] the in-region offsets of a locus' kept reads, packed from mismatch_off[r0] on
  uint64_t stage_cap;
};
template <bool SNV> using DeepClFlankArgsOf = std::conditional_t<SNV, DeepClSnvArgs, DeepClFlankArgs>;

struct DeepClFlank {
  uint32_t ln[MAXR]; uint64_t off[MAXR];  // kept reads in kept order: length and blob offset of the repeat segment
  uint64_t hash[MAXR];                    // of the segment's bytes (equal segments have equal hashes; the bytes decide)
  uint32_t ucnt[MAXR];                    // at a sequence's first read: its multiplicity inside group 0 (low half) and group 1 (high half); 0 elsewhere
  uint8_t grp[MAXR];                      // the assignment (SNV forms, a split by SNVs: bit 0 the assignment, bit 1 set for a read of both groups)
  int32_t cand[DW];                       // per thread: its smallest candidate sequence in byte order
  uint32_t med[2][2];                     // the two middle lengths of either group
  Red red;
  gt::Reserved rsv;
};
static_assert(sizeof(DeepClFlank) <= 64 * 1024, "static LDS of deep_cluster_flank_kernel");
static_assert(MAXR < 65536, "two 16-bit multiplicities share a word of DeepClFlank::ucnt");
// The search of the SNV forms runs before ln / off / hash / ucnt are filled: the offsets whose rank is taken lie over ln, its small lists
// over hash
static_assert(sizeof(int32_t) * MAXR <= sizeof(DeepClFlank::ln) && sizeof(gtd::DeepSnv) <= sizeof(DeepClFlank::hash) && offsetof(DeepClFlank, hash) % alignof(gtd::DeepSnv) == 0,
              "the search's keys and lists lie over ln and hash");

__device__ __forceinline__ void hand_back(const DeepClFlankArgs& a, int64_t l, uint8_t why = 0) {
  if (threadIdx.x == 0) { a.d.c.g.need_host[l] = 1; a.flank_done[l] = gt::FL_HANDED | why; atomicAdd(a.fcounts + DF_FAILED, 1u); }
}
// How gtd::deep_snv_search ends behind the deep cluster chain, clf::ClusterEnd for the workgroup.  true: the reads split, cnt holds the
// members and hap the assigned reads of either group; false: the byte of the locus says why not
struct DeepClusterEnd {
  const DeepClSnvArgs& a; int64_t l; int n; const uint8_t* grp; Red& red;
  int cnt[2], hap[2];
  __device__ __forceinline__ bool nosplit() const { if (threadIdx.x == 0) a.flank_done[l] = gt::FL_NOSPLIT | gt::FL_SNV; return false; }
  __device__ __forceinline__ bool handed(uint8_t why) const { hand_back(a, l, (uint8_t)(gt::FL_SNV | why)); return false; }
  __device__ __forceinline__ bool split(const int (&members)[2]) {
    if (members[0] == 0 || members[1] == 0) return nosplit();  // an empty group: no split
    uint32_t ones = 0;
    for (int i = threadIdx.x; i < n; i += DW) ones += grp[i] & 1u;
    ones = cld::block_sum_u32(ones, red);
    cnt[0] = members[0]; cnt[1] = members[1]; hap[1] = (int)ones; hap[0] = n - (int)ones;
    return true;
  }
};

// 64-bit hash of a byte string anywhere in global memory, by one thread: eight bytes a step, the tail byte by byte
__device__ __forceinline__ uint64_t hash_seg(const uint8_t* __restrict__ p, uint32_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
  auto mix = [&](uint64_t w) { h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 29; };
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) { uint64_t w; __builtin_memcpy(&w, p + i, 8); mix(w); }
  uint64_t w = 0;
  for (uint32_t s = 0; i < n; ++i, s += 8) w |= (uint64_t)p[i] << s;
  mix(w);
  return h;
}

// The end of both kernels, clf::flank_write for the workgroup: smaller allele first (genotype_flank.rs:33-38: a swap on strict >, the
// assignment flips with it), the assignment is the classification and its counts are num_spanning, reference allele first (tr.rs:95-101),
// TrSize::size = allele length.  ap / aln / civ / hap are per group -- hap: the reads assigned to it (by tags: its members; by SNVs a read
// of both groups is assigned to one) --, grp holds the assignment of the kept reads (BY_SNV: in bit 0).  mark: FL_SNV for the SNV branch,
// 0 for the tags'.  Uniform arguments.
template <bool BY_SNV = false>
__device__ __forceinline__ void deep_flank_write(const DeepClFlankArgs& a, const uint8_t* grp, int64_t l, uint64_t r0, int n, const uint8_t* const (&ap)[2], const uint32_t (&aln)[2],
                                                 const int32_t (&civ)[4], const int32_t (&hap)[2], uint8_t done, uint8_t mark = 0) {
  const gt::GtArgs& g = a.d.c.g;
  const int tid = threadIdx.x;
  // (constant indices throughout, selections instead of indexed loads: the small per-group arrays stay in registers)
  const bool sw = aln[0] > aln[1];
  const uint8_t* const p_lo = sw ? ap[1] : ap[0]; const uint32_t n_lo = sw ? aln[1] : aln[0];  // the smaller allele, or the first of two equal ones
  const uint8_t* const p_hi = sw ? ap[0] : ap[1]; const uint32_t n_hi = sw ? aln[0] : aln[1];
  const uint8_t* ref = g.tr_blob + g.tr_off[l]; const uint32_t refn = g.tr_len[l];
  // (wave_equal: every wave compares the whole strings, all reach the same answer)
  const bool flip = !gt::wave_equal(p_lo, n_lo, ref, refn) && gt::wave_equal(p_hi, n_hi, ref, refn);
  if (aln[0] > g.allele_cap[l] || aln[1] > g.allele_cap[l]) { hand_back(a, l, mark); return; }  // the host path reports the error
  const bool first1 = sw != flip;  // output allele 0 is tag group 1's
#pragma unroll
  for (int oi = 0; oi < 2; ++oi) {
    const bool g1 = (oi == 0) == first1;  // the tag group written in place oi
    const uint8_t* const src = g1 ? ap[1] : ap[0]; const uint32_t len = g1 ? aln[1] : aln[0];
    uint8_t* dst = g.allele_blob + g.allele_off[2 * l + oi];
    for (uint32_t b = tid; b < len; b += DW) dst[b] = src[b];
    if (tid == 0) {
      g.allele_len[2 * l + oi] = len;
      g.ci[4 * l + 2 * oi] = g1 ? civ[2] : civ[0]; g.ci[4 * l + 2 * oi + 1] = g1 ? civ[3] : civ[1];
      g.num_spanning[2 * l + oi] = g1 ? hap[1] : hap[0];
      if (g.gt_size) g.gt_size[2 * l + oi] = (int32_t)len;
    }
  }
  const uint8_t first_group = first1 ? 1 : 0;
  for (int i = tid; i < n; i += DW) {
    const uint32_t rd = a.d.sel_read[r0 + i];
    if constexpr (BY_SNV) g.classification[r0 + rd] = (grp[i] & 1u) == first_group ? 0 : 1;
    else g.classification[r0 + rd] = grp[i] == first_group ? 0 : 1;
    g.read_rank[r0 + rd] = i;
  }
  if (tid == 0) { g.n_alleles[l] = 2; g.n_spanning_reads[l] = (uint32_t)n; g.flipped[l] = (uint8_t)flip; a.flank_done[l] = done | mark; }
}

template <bool SNV = false>
__global__ void __launch_bounds__(DW) deep_cluster_flank_kernel(const DeepClFlankArgsOf<SNV> a) {
  using MEM = gtd::DeepSnvMembers;  // (SNV forms, a split by SNVs) who belongs to a group, from the byte in grp
  __shared__ DeepClFlank sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.d.c.n_list) return;
  const gt::GtArgs& g = a.d.c.g;
  const int64_t l = a.d.c.list[k];
  const int tid = threadIdx.x;
  if (tid == 0) a.flank_done[l] = 0;  // (no other kernel writes the byte of a deep cluster locus)
  // only a locus deep_finish_kernel completed, with two alleles at most 10 apart (tr.rs:69-75; the cluster genotyper's sizes are its allele
  // lengths, and the difference does not depend on the reference-first swap)
  const cl::ClRec rec = a.d.c.rec[k];
  if (rec.state != 1 || g.need_host[l] != 0 || g.n_alleles[l] != 2) return;
  if (gt::adiff_u(g.allele_len[2 * l], g.allele_len[2 * l + 1]) > 10) return;
  const uint64_t r0 = g.locus_read_begin[l];
  const int n = rec.n;
  if (n <= 0 || n > MAXR) return;
  int cnt[2];  // members of either group
  int hap[2] = {0, 0};  // (SNV forms) the reads assigned to it: by tags its members, by SNVs a read of both groups is assigned to one
  bool snv = false;     // (SNV forms) the split is the SNV branch's: its groups overlap
  if constexpr (!SNV) {
    if (!gtd::deep_flank_assign(sh.grp, a.d, a.hp_tag, r0, n, cnt, sh.red)) return;  // the tags do not split the reads: the host tries the SNV branch as before
  } else {
    if (a.hp_tag && gtd::deep_flank_assign(sh.grp, a.d, a.hp_tag, r0, n, cnt, sh.red)) {
      if (!a.tag_route) return;  // the tags own the locus and the host finds their split as before: the byte stays 0
      hap[0] = cnt[0]; hap[1] = cnt[1];
    } else {
      // the search, before ln / off / hash / ucnt are filled: its keys over ln, its lists over hash (kept read i is read r0 + sel_read[r0 + i]
      // of the batch, as in the deep size route)
      DeepClusterEnd end{a, l, n, sh.grp, sh.red, {0, 0}, {0, 0}};
      if (!gtd::deep_snv_search(*reinterpret_cast<gtd::DeepSnv*>(static_cast<void*>(sh.hash)), reinterpret_cast<int32_t*>(sh.ln), sh.grp, sh.red, a, r0, n,
                                [&](int i) { return r0 + a.d.sel_read[r0 + i]; }, end))
        return;  // no split, or handed back: the byte says which
      cnt[0] = end.cnt[0]; cnt[1] = end.cnt[1]; hap[0] = end.hap[0]; hap[1] = end.hap[1];
      snv = true;
    }
  }
  const uint8_t mark = snv ? (uint8_t)gt::FL_SNV : (uint8_t)0;
  // (the tag forms keep the statements they had, here and below: their resource figures stay; profiles/snv_cluster_deep_resource_usage.txt)
  auto in = [&](uint32_t b, int q) {  // a read whose byte in grp is b is a member of group q
    if constexpr (SNV) return snv ? MEM::in(b, q) : b == (uint32_t)q;
    else return b == (uint32_t)q;
  };
  // ---- every thread reads the segments of its reads once: length, offset, hash
  for (int i = tid; i < n; i += DW) {
    const uint32_t li = a.d.sel_len[r0 + i];
    const uint64_t oi = cld::seg_off(a.d, r0, i);
    sh.ln[i] = li; sh.off[i] = oi; sh.hash[i] = hash_seg(g.reads + oi, li); sh.ucnt[i] = 0;
  }
  __syncthreads();
  auto seg_of = [&](int i) { return gt::Seg{sh.off[i], sh.ln[i]}; };
  auto seg_ptr = [&](int i) { return g.reads + sh.off[i]; };
  {
    // ---- all pairs, on LDS: thread t owns reads t, t + DW, ...; against every read j in kept order
    //      first[x]: the first kept read with the sequence of read x (bytes compared where length and hash agree, until one is found)
    //      rk[x]:    the rank of read x among the lengths of its group, #{shorter} + #{equal and earlier}
    //      (SNV forms: a read of both groups has a rank in either -- rk among the members of group 0, rk1 among those of group 1)
    uint32_t li[DT]; uint64_t hi[DT]; uint32_t gi[DT]; int rk[DT], first[DT];
    int rk1[SNV ? DT : 1]; (void)rk1;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int i = tid + DW * t;
      const bool valid = i < n;
      li[t] = valid ? sh.ln[i] : 0xFFFFFFFFu; hi[t] = valid ? sh.hash[i] : 0ull; gi[t] = valid ? (uint32_t)sh.grp[i] : 2u;
      rk[t] = 0; first[t] = i;
      if constexpr (SNV) rk1[t] = 0;
    }
    for (int j = 0; j < n; ++j) {
      const uint32_t lj = sh.ln[j]; const uint64_t hj = sh.hash[j]; const uint32_t gj = sh.grp[j];
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const int i = tid + DW * t;
        if constexpr (SNV) {
          const bool before = lj < li[t] || (lj == li[t] && j < i);
          rk[t] += in(gj, 0) && before; rk1[t] += in(gj, 1) && before;
        } else rk[t] += gj == gi[t] && (lj < li[t] || (lj == li[t] && j < i));
        if (lj == li[t] && hj == hi[t] && j < i && first[t] == i && gtd::cmp_seg_thread(seg_ptr(j), lj, seg_ptr(i), lj) == 0) first[t] = j;
      }
    }
    // ---- multiplicities inside the groups, counted at a sequence's first read (integer sums: the order does not matter); the two middle
    //      lengths of either group
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      if (tid + DW * t >= n) continue;
      if constexpr (SNV) {  // a read of both groups counts in both halves, and can be a middle element of either
        const bool in0 = in(gi[t], 0), in1 = in(gi[t], 1);
        atomicAdd(&sh.ucnt[first[t]], (in0 ? 1u : 0u) + (in1 ? 0x10000u : 0u));
        if (in0 && rk[t] == cnt[0] / 2) sh.med[0][1] = li[t];
        if (in0 && rk[t] == cnt[0] / 2 - 1) sh.med[0][0] = li[t];
        if (in1 && rk1[t] == cnt[1] / 2) sh.med[1][1] = li[t];
        if (in1 && rk1[t] == cnt[1] / 2 - 1) sh.med[1][0] = li[t];
      } else {
        const int q = (int)gi[t];
        atomicAdd(&sh.ucnt[first[t]], q ? 0x10000u : 1u);
        if (rk[t] == cnt[q] / 2) sh.med[q][1] = li[t];
        if (rk[t] == cnt[q] / 2 - 1) sh.med[q][0] = li[t];
      }
    }
  }
  __syncthreads();
  // ---- simple_consensus (:154-169) of either group
  int rep[2]; uint32_t aln[2]; int32_t civ[4]; bool lacks[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {  // (unrolled here and below: the small per-group arrays stay in registers)
    auto mult = [&](int i) { return q ? sh.ucnt[i] >> 16 : sh.ucnt[i] & 0xFFFFu; };
    // utils::math::median (math.rs:73-98) as f32, truncated: the middle value, or (a + b) as i32, then / 2.0
    const float med = (cnt[q] & 1) ? (float)(int32_t)sh.med[q][1] : (float)((int32_t)sh.med[q][0] + (int32_t)sh.med[q][1]) / 2.0f;
    const uint32_t median_len = (uint32_t)med;
    uint32_t top = 0, bd = 0xFFFFFFFFu, mn = 0xFFFFFFFFu, mx = 0;
    for (int i = tid; i < n; i += DW) { const uint32_t m = mult(i); top = m > top ? m : top; }
    top = gtd::block_max_u32(top, sh.red);
    for (int i = tid; i < n; i += DW) if (mult(i) == top) { const uint32_t d = gt::adiff_u(sh.ln[i], median_len); bd = d < bd ? d : bd; }
    bd = gtd::block_min_u32(bd, sh.red);
    // among the sequences of the largest multiplicity the first minimum of |len - median| in BTreeMap order: of those at the minimum, the
    // smallest in byte order, a proper prefix first (not the first in read order).  The candidates are distinct sequences, so the minimum
    // is one read whichever thread looked at it: first inside each thread, then a tree over the threads
    int best = -1;
    for (int i = tid; i < n; i += DW)
      if (mult(i) == top && gt::adiff_u(sh.ln[i], median_len) == bd && (best < 0 || gtd::cmp_seg_thread(seg_ptr(i), sh.ln[i], seg_ptr(best), sh.ln[best]) < 0)) best = i;
    sh.cand[tid] = best;
    __syncthreads();
    for (int s = DW / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const int x = sh.cand[tid], y = sh.cand[tid + s];
        if (y >= 0 && (x < 0 || gtd::cmp_seg_thread(seg_ptr(y), sh.ln[y], seg_ptr(x), sh.ln[x]) < 0)) sh.cand[tid] = y;
      }
      __syncthreads();
    }
    best = sh.cand[0];  // (the group is not empty: some thread had a candidate)
    if (best < 0) { hand_back(a, l, mark); return; }  // (cannot happen; uniform, and no index below is taken from a value that was never set)
    for (int i = tid; i < n; i += DW) if (in(sh.grp[i], q)) { const uint32_t v = sh.ln[i]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    civ[2 * q] = (int32_t)gtd::block_min_u32(mn, sh.red); civ[2 * q + 1] = (int32_t)gtd::block_max_u32(mx, sh.red);  // (their barriers: cand is free again)
    rep[q] = best; aln[q] = sh.ln[best];
    lacks[q] = (double)top / (double)cnt[q] < 0.5;
  }
  if (!lacks[0] && !lacks[1]) {
    const uint8_t* const ap[2] = {seg_ptr(rep[0]), seg_ptr(rep[1])};
    if constexpr (SNV) deep_flank_write<true>(a, sh.grp, l, r0, n, ap, aln, civ, hap, (uint8_t)gt::FL_DONE, mark);
    else deep_flank_write(a, sh.grp, l, r0, n, ap, aln, civ, cnt, (uint8_t)gt::FL_DONE);
    return;
  }
  // ---- a group below 50 %: backbone = its sequence, one member per read of the group in kept order, duplicates included.  The arenas
  //      first; no job or group slot is taken unless all three fit
  uint32_t nm[2] = {0, 0}; unsigned long long mbytes[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (!lacks[q]) continue;
    uint32_t bytes = 0;
    for (int i = tid; i < n; i += DW) if (in(sh.grp[i], q)) bytes += sh.ln[i];
    nm[q] = (uint32_t)cnt[q]; mbytes[q] = cld::block_sum_u32(bytes, sh.red);
  }
  gt::GroupNeeds nd[2] = {};
#pragma unroll
  for (int q = 0; q < 2; ++q) if (lacks[q]) nd[q] = gt::group_needs(aln[q], nm[q], mbytes[q], a.d.c.vote_lds_pos);
  if (tid == 0) {
    gt::Reserved r;
    r.g0 = r.j0 = 0;
    if (gt::reserve_arenas(a.d.c.counts + cl::CC_CIGAR, a.d.c.counts + cl::CC_OUT, a.d.c.counts + cl::CC_SCRATCH, a.d.c.cap_cigar, a.d.c.cap_out, a.d.c.cap_scratch, nd, r)) {
      // (room in the third part of the lists: a read is a member of one tag group, of at most two SNV groups -- cap_j jobs for the launch
      //  of the tag forms, 2 cap_j for that of the SNV forms, which is how cluster_chain sizes the lists; 2 groups per locus)
      r.j0 = a.first_job + atomicAdd(a.fcounts + DF_J3, nm[0] + nm[1]);
      r.g0 = a.first_group + atomicAdd(a.fcounts + DF_G3, (uint32_t)lacks[0] + (uint32_t)lacks[1]);
    }
    sh.rsv = r;
  }
  __syncthreads();
  if (!sh.rsv.ok) { hand_back(a, l, mark); return; }
  gt::Reserved at = sh.rsv;
  clf::ClFlankPend pd;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const gt::Seg s = seg_of(rep[q]);
    pd.bb_off[q] = s.off; pd.bb_len[q] = s.len; pd.civ[2 * q] = civ[2 * q]; pd.civ[2 * q + 1] = civ[2 * q + 1]; pd.cnt[q] = cnt[q]; pd.grp[q] = -1;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (lacks[q]) pd.grp[q] = (int32_t)gt::queue_group<DW>(a.d.c.groups, a.d.c.jobs, at, seg_of(rep[q]), nm[q], nd[q], n, [&, q](int i) { return in(sh.grp[i], q); }, seg_of);
  // (SNV forms: a waiting locus of the SNV branch has its split in snv_read, where the search left it; the finish kernel reads it and does not
  //  repeat the search)
  if constexpr (SNV) { if (snv && tid == 0) { a.pend_hap[2 * k] = hap[0]; a.pend_hap[2 * k + 1] = hap[1]; } }
  if (tid == 0) { a.pend[k] = pd; a.flank_done[l] = gt::FL_REPAIRED | mark; }  // the locus waits for deep_cluster_flank_finish_kernel
}

// ---- behind the third consensus round: the loci that waited.  The assignment is recomputed from the tags (deterministic from the same
// list of kept reads); each allele is the voted consensus of a repaired group or the backbone of a group that needed none.
// (SNV forms: a locus of the SNV branch waits with FL_REPAIRED | FL_SNV; its assignment is read back from snv_read, its counts from pend
// and pend_hap)
struct DeepClFlankFin { uint8_t grp[MAXR]; Red red; };
template <bool SNV = false>
__global__ void __launch_bounds__(DW) deep_cluster_flank_finish_kernel(const DeepClFlankArgsOf<SNV> a) {
  __shared__ DeepClFlankFin sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.d.c.n_list) return;
  const gt::GtArgs& g = a.d.c.g;
  const int64_t l = a.d.c.list[k];
  bool snv = false;
  if constexpr (SNV) snv = a.flank_done[l] == (gt::FL_REPAIRED | gt::FL_SNV);
  if (a.flank_done[l] != gt::FL_REPAIRED && !snv) return;  // (thread 0 writes the byte behind the barriers of the assignment: every thread has read it by then)
  const uint64_t r0 = g.locus_read_begin[l];
  const int n = a.d.c.rec[k].n;
  const clf::ClFlankPend pd = a.pend[k];
  int cnt[2] = {0, 0};
  int32_t hap[2] = {0, 0};  // (SNV forms) the assigned reads of either group of a locus of the SNV branch
  bool fail = n <= 0 || n > MAXR;
  if constexpr (SNV) {
    if (snv) {
      if (!fail) for (int i = threadIdx.x; i < n; i += DW) sh.grp[i] = (uint8_t)(a.snv_read[r0 + i] & gt::SR_ASSIGN);
      hap[0] = a.pend_hap[2 * k]; hap[1] = a.pend_hap[2 * k + 1];
      __syncthreads();  // (grp is visible, and every thread has read the byte)
      if (!fail) fail = n != hap[0] + hap[1];
    } else if (!fail) fail = !gtd::deep_flank_assign(sh.grp, a.d, a.hp_tag, r0, n, cnt, sh.red) || cnt[0] != pd.cnt[0] || cnt[1] != pd.cnt[1];
  } else {
    if (!fail) fail = !gtd::deep_flank_assign(sh.grp, a.d, a.hp_tag, r0, n, cnt, sh.red) || cnt[0] != pd.cnt[0] || cnt[1] != pd.cnt[1];
  }
  const uint8_t mark = snv ? (uint8_t)gt::FL_SNV : (uint8_t)0;
  const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0};
  for (int q = 0; q < 2 && !fail; ++q) {
    if (pd.grp[q] >= 0) {
      const uint32_t voted = a.d.c.vote_len[pd.grp[q]];
      if (voted == 0xFFFFFFFFu) { fail = true; break; }  // the vote gave up on the group (overflow of its result slot)
      ap[q] = a.d.c.vote_out + a.d.c.groups[pd.grp[q]].out_off; aln[q] = voted;
    } else { ap[q] = g.reads + pd.bb_off[q]; aln[q] = pd.bb_len[q]; }
  }
  if (fail) { hand_back(a, l, mark); return; }
  const uint8_t* const apc[2] = {ap[0], ap[1]};
  if constexpr (SNV) {
    if (snv) deep_flank_write<true>(a, sh.grp, l, r0, n, apc, aln, pd.civ, hap, (uint8_t)(gt::FL_DONE | gt::FL_REPAIRED), mark);
    else deep_flank_write<true>(a, sh.grp, l, r0, n, apc, aln, pd.civ, pd.cnt, (uint8_t)(gt::FL_DONE | gt::FL_REPAIRED));
  } else deep_flank_write(a, sh.grp, l, r0, n, apc, aln, pd.civ, pd.cnt, (uint8_t)(gt::FL_DONE | gt::FL_REPAIRED));
}

}  // namespace cldf
}  // namespace trgt
