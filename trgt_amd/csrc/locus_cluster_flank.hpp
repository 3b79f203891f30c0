// trgt_amd/csrc/locus_cluster_flank.hpp -- the haplotype-tag branch of genotype_flank::genotype (genotype_flank.rs:9-76, 147-170) for
// Genotyper::Cluster loci, behind the one-wave cluster chain of locus_cluster_dev.hpp.  analyze (tr.rs:64-75) re-genotypes every diploid
// locus whose two alleles are at most 10 bases apart, whichever genotyper produced them; for the size genotyper the FLANK forms of
// locus_gt.hpp do that inside the genotype kernel, for a cluster locus the host redid the locus from the start.  On a context that opted
// in (trgt_hip_set_flank_cluster_device), for a batch with haplotype tags, two kernels follow cluster_finish_kernel:
//   cluster_flank_kernel          a locus the chain completed with two alleles at most 10 apart: assignment by tag (gt::flank_assign),
//                                 simple_consensus of either group; without a group below 50 % the locus is settled here, else the groups
//                                 are queued (repair_queue.hpp) for a THIRD consensus round of the chain -- BiWFA + consensus_vote_kernel
//                                 over the third part of the job and group lists -- and the locus waits (flank_done = FL_REPAIRED)
//   cluster_flank_finish_kernel   the waiting loci: alleles = voted consensus or backbone, same order and outputs
// One wave per locus of the shallow list (at most GT_MAX_READS reads).  The cluster chain has no sequence histogram: equal segments are
// found where they lie, in the read blob.  A locus whose tags do not split its reads is not touched -- the host sees it as before and
// tries the SNV branch; one that finds no room in the arenas, whose vote overflows or whose allele exceeds allele_cap is handed back
// (need_host = 1, FL_HANDED) and takes the host path.  The kernels of locus_cluster_dev.hpp are used as they are.
// The SNV forms of the two kernels (contexts that opted in with trgt_hip_set_snv_cluster_device, batches that carry mismatch offsets) add
// the other branch, get_trs_with_clustering (genotype_flank.rs:78-138, 171-290), in the reference's order: tags that split the reads own
// the locus (this route with both settings on, else the host as before: the byte stays 0), and only without such tags the search of
// gt::snv_route runs -- the one of the size genotyper's SNV forms, with its limits and its margin rule (locus_gt.hpp).  Its groups
// overlap: a read that agrees equally with both haplotypes is a member of both (gt::SnvMembers) while its assignment alternates.  The
// multiplicities, the medians, the 50 % test, the intervals and the third round's members follow the membership, num_spanning and the
// classification the assignment.  The bytes carry FL_SNV: FL_NOSPLIT (the host need not look again), FL_DONE, or FL_HANDED (limits,
// FL_UNDECIDED, and the hand-backs of the tag route).
#pragma once
#include "locus_cluster_dev.hpp"

namespace trgt {
namespace clf {

// the route's own count block (the chain's CC_* block keeps its layout; the arenas are the chain's, CC_CIGAR / CC_OUT / CC_SCRATCH)
enum { CF_J3 = 0 /* jobs of the third round */, CF_G3 = 1 /* vote groups */, CF_FAILED = 2 /* loci handed back */, CF_WORDS = 16 };

struct ClFlankPend {  // what cluster_flank_kernel had decided for a locus that waits for the third round
  uint64_t bb_off[2]; uint32_t bb_len[2];  // the backbones (segments of the read blob)
  int32_t civ[4];                          // (min, max) segment length of either group
  int32_t cnt[2];                          // members
  int32_t grp[2];                          // vote group, -1: the backbone stands
};

// ClArgs is part of every cluster and deep kernel's arguments and does not grow: what the two kernels read beyond it
struct ClFlankArgs {
  cl::ClArgs c;
  const int16_t* hp_tag;  // per read of the batch: the HP tag (-1 = None)
  uint8_t* flank_done;    // [n_loci] gt::FL_*, written for the loci of the list only
  uint32_t* fcounts;      // [CF_WORDS]
  ClFlankPend* pend;      // [n_list]
  uint32_t first_job, first_group;  // the third part of the chain's job and group lists
};

template <int MAXR>
struct ClFlankShared {
  uint32_t r_s[MAXR], r_len[MAXR]; uint64_t r_off[MAXR];
  uint32_t s_read[MAXR], s_start[MAXR], s_len[MAXR];
  int8_t cls[MAXR];         // the assignment
  uint16_t uid[MAXR];       // per kept read: the first kept read with the same sequence
  uint16_t ucnt[2][MAXR];   // at a sequence's first read: its multiplicity inside either group (0 elsewhere)
  uint32_t med[2][2];       // the two middle lengths of either group
  gt::Reserved rsv;
  int n;
};

// ... and what the SNV forms read beyond that (a struct of its own: ClFlankArgs does not grow)
struct ClSnvArgs : ClFlankArgs {
  const int32_t *start_offset, *end_offset;  // per read of the batch (NULL = 0 for every read, as in flank_split)
  const int32_t* mismatch_offsets; const uint64_t* mismatch_off;  // per read r: its ascending offsets in [mismatch_off[r], mismatch_off[r + 1])
  uint8_t* snv_read;      // per read slot of the batch, by position in the kept list: gt::SR_* of a locus that waits for the third round
  int32_t* pend_hap;      // [2 n_list] beside pend: the assigned reads of either group (ClFlankPend::cnt holds the members)
  double ln_match, ln_mis, ln2;  // ln 0.9, ln(1.0 - 0.9), ln 2 as the host's libm rounds them
  int32_t tag_route;      // 1: tags that split the reads are this route's (trgt_hip_set_flank_cluster_device is on as well); 0: the host's
};
template <bool SNV> using ClFlankArgsOf = std::conditional_t<SNV, ClSnvArgs, ClFlankArgs>;
template <int MAXR, bool SNV> struct ClFlankSharedOf : ClFlankShared<MAXR> {};
template <int MAXR> struct ClFlankSharedOf<MAXR, true> : ClFlankShared<MAXR>, gt::SnvShared<MAXR, true> {  // 9 + 10.9 KB for 256 reads
  int snv_cnt[2], snv_hap[2];  // what the search found: members / assigned reads of either group
};

__device__ __forceinline__ void hand_back(const ClFlankArgs& a, int64_t l, int lane, uint8_t why = 0) {
  if (lane == 0) { a.c.g.need_host[l] = 1; a.flank_done[l] = gt::FL_HANDED | why; atomicAdd(a.fcounts + CF_FAILED, 1u); }
}
// How gt::snv_route ends behind the cluster chain.  true: the reads split, and the counts are in sh.snv_cnt / sh.snv_hap; false: the byte
// of the locus says why not
struct ClusterEnd {
  static constexpr bool SIZE = false;
  template <class SH> static __device__ __forceinline__ bool nosplit(SH&, const ClSnvArgs& a, int64_t l, int lane) { if (lane == 0) a.flank_done[l] = gt::FL_NOSPLIT | gt::FL_SNV; return false; }
  template <class SH> static __device__ __forceinline__ bool handed(SH&, const ClSnvArgs& a, int64_t l, int lane, uint8_t why) { hand_back(a, l, lane, (uint8_t)(gt::FL_SNV | why)); return false; }
  template <class SH> static __device__ __forceinline__ bool split(SH& sh, const ClSnvArgs& a, int64_t l, int lane, const int* cnt, const int* hap) {
    if (cnt[0] == 0 || cnt[1] == 0) return nosplit(sh, a, l, lane);  // an empty group: no split
    if (lane == 0) { sh.snv_cnt[0] = cnt[0]; sh.snv_cnt[1] = cnt[1]; sh.snv_hap[0] = hap[0]; sh.snv_hap[1] = hap[1]; }
    __syncthreads();
    return true;
  }
};

// The end of both kernels: smaller allele first (genotype_flank.rs:33-38: a swap on strict >, the assignment flips with it), the
// assignment is the classification and its counts are num_spanning, reference allele first (tr.rs:95-101), TrSize::size = allele length.
// ap / aln / civ / hap are per group -- hap: the reads assigned to it (by tags: its members; by SNVs a read of both groups is assigned to
// one); sh.cls holds the assignment.  mark: FL_SNV for the SNV branch, 0 for the tags'.  Uniform arguments.
template <class SH>
__device__ __forceinline__ void flank_write(SH& sh, const ClFlankArgs& a, int64_t l, uint64_t r0, int n, int lane, const uint8_t* const (&ap)[2], const uint32_t (&aln)[2],
                                            const int32_t (&civ)[4], const int32_t (&hap)[2], uint8_t done, uint8_t mark = 0) {
  const gt::GtArgs& g = a.c.g;
  const int sw = aln[0] > aln[1] ? 1 : 0;
  int order[2] = {sw, 1 - sw}, flip = 0;  // output allele -> tag group
  const uint8_t* ref = g.tr_blob + g.tr_off[l]; const uint32_t refn = g.tr_len[l];
  if (!gt::wave_equal(ap[order[0]], aln[order[0]], ref, refn) && gt::wave_equal(ap[order[1]], aln[order[1]], ref, refn)) { order[0] = 1 - sw; order[1] = sw; flip = 1; }
  if (aln[0] > g.allele_cap[l] || aln[1] > g.allele_cap[l]) { hand_back(a, l, lane, mark); return; }  // the host path reports the error
  for (int oi = 0; oi < 2; ++oi) {
    const int q = order[oi];
    uint8_t* dst = g.allele_blob + g.allele_off[2 * l + oi];
    for (uint32_t b = lane; b < aln[q]; b += 64) dst[b] = ap[q][b];
    if (lane == 0) {
      g.allele_len[2 * l + oi] = aln[q];
      g.ci[4 * l + 2 * oi] = civ[2 * q]; g.ci[4 * l + 2 * oi + 1] = civ[2 * q + 1];
      g.num_spanning[2 * l + oi] = hap[q];
      if (g.gt_size) g.gt_size[2 * l + oi] = (int32_t)aln[q];
    }
  }
  for (int i = lane; i < n; i += 64) {
    g.classification[r0 + sh.s_read[i]] = sh.cls[i] == order[0] ? 0 : 1;
    g.read_rank[r0 + sh.s_read[i]] = i;
  }
  if (lane == 0) { g.n_alleles[l] = 2; g.n_spanning_reads[l] = (uint32_t)n; g.flipped[l] = (uint8_t)flip; a.flank_done[l] = done | mark; }
}

template <int MAXR, bool PRESEL = false, bool SNV = false>
__global__ void __launch_bounds__(64) cluster_flank_kernel(const ClFlankArgsOf<SNV> a) {
  __shared__ ClFlankSharedOf<MAXR, SNV> sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const gt::GtArgs& g = a.c.g;
  const int64_t l = a.c.list[k];
  const int lane = threadIdx.x;
  if (lane == 0) a.flank_done[l] = 0;  // (no other kernel clears the byte of a cluster locus on a context with this setting alone)
  // only a locus cluster_finish_kernel completed, with two alleles at most 10 apart (tr.rs:69-75; the cluster genotyper's sizes are its
  // allele lengths, and the difference does not depend on the reference-first swap)
  if (a.c.rec[k].state != 1 || g.need_host[l] != 0 || g.n_alleles[l] != 2) return;
  if (gt::adiff_u(g.allele_len[2 * l], g.allele_len[2 * l + 1]) > 10) return;
  const uint64_t r0 = g.locus_read_begin[l];
  const int nr = (int)(g.locus_read_begin[l + 1] - r0);
  if (nr > MAXR) return;
  if (lane == 0) sh.n = 0;
  gt::gt_selected<MAXR, PRESEL>(sh, g, l, r0, nr, lane);
  const int n = sh.n;
  if (n == 0) return;
  int cnt[2];           // members of either group
  int hap[2] = {0, 0};  // (SNV forms) the reads assigned to it: by tags its members, by SNVs a read of both groups is assigned to one
  bool snv = false;     // (SNV forms) the split is the SNV branch's: its groups overlap
  if constexpr (!SNV) {
    if (!gt::flank_assign(sh, a.hp_tag, r0, n, lane, cnt)) return;  // the tags do not split the reads: the host tries the SNV branch as before
  } else {
    if (a.hp_tag && gt::flank_assign(sh, a.hp_tag, r0, n, lane, cnt)) {
      if (!a.tag_route) return;  // the tags own the locus and the host finds their split as before: the byte stays 0
      hap[0] = cnt[0]; hap[1] = cnt[1];
    } else {
      if (!gt::snv_route<MAXR, ClusterEnd>(sh, a, l, r0, n, 0, lane, false, 0u, 0ull)) return;  // no split, or handed back: the byte says which
      cnt[0] = sh.snv_cnt[0]; cnt[1] = sh.snv_cnt[1]; hap[0] = sh.snv_hap[0]; hap[1] = sh.snv_hap[1];
      snv = true;
    }
  }
  const uint8_t mark = snv ? (uint8_t)gt::FL_SNV : (uint8_t)0;
  // (the tag forms keep the statements they had, below and where flank_write is called: written through in() or with a copy of cnt their
  //  figures move -- SGPR spills of cluster_flank_kernel, VGPRs of the finish kernel; profiles/snv_cluster_resource_usage.txt)
  auto in = [&](int i, int q) {  // read i is a member of group q
    if constexpr (SNV) return sh.cls[i] == q || (snv && sh.v_tie[i]);
    else return sh.cls[i] == q;
  };
  auto seg_of = [&](int i) { return gt::Seg{sh.r_off[sh.s_read[i]] + sh.s_start[i], sh.s_len[i]}; };
  auto seg_ptr = [&](int i) { return g.reads + sh.r_off[sh.s_read[i]] + sh.s_start[i]; };
  // ---- equal sequences: one lane per read against the earlier reads, lengths first, then the bytes where they lie
  for (int i = lane; i < n; i += 64) {
    const uint32_t li = sh.s_len[i];
    const uint8_t* pi = seg_ptr(i);
    int u = i;
    for (int j = 0; j < i; ++j) {
      if (sh.s_len[j] != li) continue;
      const uint8_t* pj = seg_ptr(j);
      uint32_t b = 0;
      while (b < li && pi[b] == pj[b]) ++b;
      if (b == li) { u = j; break; }
    }
    sh.uid[i] = (uint16_t)u;
  }
  __syncthreads();
  // ---- multiplicities inside the groups (at the first read of every sequence), and the middle lengths of either group by rank
  for (int i = lane; i < n; i += 64) {
    int c0 = 0, c1 = 0;
    if (sh.uid[i] == i)
      for (int j = i; j < n; ++j) if (sh.uid[j] == i) {
        if constexpr (SNV) { c0 += in(j, 0); c1 += in(j, 1); }
        else { if (sh.cls[j]) ++c1; else ++c0; }
      }
    sh.ucnt[0][i] = (uint16_t)c0; sh.ucnt[1][i] = (uint16_t)c1;
    if constexpr (SNV) {  // a middle element of either group it is a member of: its rank among the lengths of the group's members
      const uint32_t li = sh.s_len[i];
      for (int q = 0; q < 2; ++q) {
        if (!in(i, q)) continue;
        int r = 0;
        for (int j = 0; j < n; ++j) { const uint32_t lj = sh.s_len[j]; r += in(j, q) && (lj < li || (lj == li && j < i)); }
        if (r == cnt[q] / 2) sh.med[q][1] = li;
        if (r == cnt[q] / 2 - 1) sh.med[q][0] = li;
      }
    } else {
      const int q = sh.cls[i]; const uint32_t li = sh.s_len[i];
      int r = 0;
      for (int j = 0; j < n; ++j) { const uint32_t lj = sh.s_len[j]; r += sh.cls[j] == q && (lj < li || (lj == li && j < i)); }
      if (r == cnt[q] / 2) sh.med[q][1] = li;
      if (r == cnt[q] / 2 - 1) sh.med[q][0] = li;
    }
  }
  __syncthreads();
  // ---- simple_consensus (:154-169) of either group
  int rep[2]; uint32_t aln[2]; int32_t civ[4]; bool lacks[2];
  for (int q = 0; q < 2; ++q) {
    // utils::math::median (math.rs:73-98) as f32, truncated: the middle value, or (a + b) as i32, then / 2.0
    const float med = (cnt[q] & 1) ? (float)(int32_t)sh.med[q][1] : (float)((int32_t)sh.med[q][0] + (int32_t)sh.med[q][1]) / 2.0f;
    const uint32_t median_len = (uint32_t)med;
    uint32_t top = 0, bd = 0xFFFFFFFFu, mn = 0xFFFFFFFFu, mx = 0;
    for (int i = lane; i < n; i += 64) top = sh.ucnt[q][i] > top ? sh.ucnt[q][i] : top;
    top = gt::wave_max_u(top);
    for (int i = lane; i < n; i += 64) if (sh.ucnt[q][i] == top) { const uint32_t d = gt::adiff_u(sh.s_len[i], median_len); bd = d < bd ? d : bd; }
    bd = gt::wave_min_u(bd);
    // among the sequences of the largest multiplicity the first minimum of |len - median| in BTreeMap order: of those at the minimum, the
    // smallest in byte order, a proper prefix first (not the first in read order)
    int best = -1;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      unsigned long long m = __ballot(i < n && sh.ucnt[q][i] == top && gt::adiff_u(sh.s_len[i], median_len) == bd);
      while (m) {
        const int cand = base + __ffsll((long long)m) - 1;
        m &= m - 1;
        if (best < 0 || gt::cmp_bytes(seg_ptr(cand), sh.s_len[cand], seg_ptr(best), sh.s_len[best]) < 0) best = cand;
      }
    }
    for (int i = lane; i < n; i += 64) if (in(i, q)) { mn = sh.s_len[i] < mn ? sh.s_len[i] : mn; mx = sh.s_len[i] > mx ? sh.s_len[i] : mx; }
    civ[2 * q] = (int32_t)gt::wave_min_u(mn); civ[2 * q + 1] = (int32_t)gt::wave_max_u(mx);
    rep[q] = best; aln[q] = sh.s_len[best];
    lacks[q] = (double)top / (double)cnt[q] < 0.5;
  }
  if (!lacks[0] && !lacks[1]) {
    const uint8_t* const ap[2] = {seg_ptr(rep[0]), seg_ptr(rep[1])};
    if constexpr (SNV) flank_write(sh, a, l, r0, n, lane, ap, aln, civ, hap, (uint8_t)gt::FL_DONE, mark);
    else flank_write(sh, a, l, r0, n, lane, ap, aln, civ, cnt, (uint8_t)gt::FL_DONE);
    return;
  }
  // ---- a group below 50 %: backbone = its sequence, one member per read of the group in kept order, duplicates included.  The arenas
  //      first; no job or group slot is taken unless all three fit
  uint32_t nm[2] = {0, 0}; unsigned long long mbytes[2] = {0, 0};
  if constexpr (SNV) { for (int i = 0; i < n; ++i) for (int q = 0; q < 2; ++q) if (lacks[q] && in(i, q)) { nm[q] += 1; mbytes[q] += sh.s_len[i]; } }
  else for (int i = 0; i < n; ++i) { const int q = sh.cls[i]; if (lacks[q]) { nm[q] += 1; mbytes[q] += sh.s_len[i]; } }
  gt::GroupNeeds nd[2] = {};
#pragma unroll
  for (int q = 0; q < 2; ++q) if (lacks[q]) nd[q] = gt::group_needs(aln[q], nm[q], mbytes[q], a.c.vote_lds_pos);
  if (lane == 0) {
    gt::Reserved r;
    if (gt::reserve_arenas(a.c.counts + cl::CC_CIGAR, a.c.counts + cl::CC_OUT, a.c.counts + cl::CC_SCRATCH, a.c.cap_cigar, a.c.cap_out, a.c.cap_scratch, nd, r)) {
      // (room in the third part of the job list: a read is a member of one tag group, of at most two SNV groups -- cap_j jobs for the
      //  launch of the tag forms, 2 cap_j for that of the SNV forms, which is how enqueue sizes the lists)
      r.j0 = a.first_job + atomicAdd(a.fcounts + CF_J3, nm[0] + nm[1]);
      r.g0 = a.first_group + atomicAdd(a.fcounts + CF_G3, (uint32_t)lacks[0] + (uint32_t)lacks[1]);
    }
    sh.rsv = r;
  }
  __syncthreads();
  if (!sh.rsv.ok) { hand_back(a, l, lane, mark); return; }
  gt::Reserved at = sh.rsv;
  ClFlankPend pd;
  for (int q = 0; q < 2; ++q) {
    const gt::Seg s = seg_of(rep[q]);
    pd.bb_off[q] = s.off; pd.bb_len[q] = s.len; pd.civ[2 * q] = civ[2 * q]; pd.civ[2 * q + 1] = civ[2 * q + 1]; pd.cnt[q] = cnt[q]; pd.grp[q] = -1;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (lacks[q]) pd.grp[q] = (int32_t)gt::queue_group<64>(a.c.groups, a.c.jobs, at, seg_of(rep[q]), nm[q], nd[q], n, [&, q](int i) { return in(i, q); }, seg_of);
  if constexpr (SNV) {
    // a waiting locus of the SNV branch leaves its split behind: the finish kernel reads it and does not repeat the search
    if (snv) {
      for (int i = lane; i < n; i += 64) a.snv_read[r0 + i] = (uint8_t)((sh.cls[i] ? gt::SR_ASSIGN : 0) | (in(i, 0) ? gt::SR_IN0 : 0) | (in(i, 1) ? gt::SR_IN1 : 0));
      if (lane == 0) { a.pend_hap[2 * k] = hap[0]; a.pend_hap[2 * k + 1] = hap[1]; }
    }
  }
  if (lane == 0) { a.pend[k] = pd; a.flank_done[l] = gt::FL_REPAIRED | mark; }  // the locus waits for cluster_flank_finish_kernel
}

// ---- behind the third consensus round: the loci that waited.  The assignment is recomputed from the tags (deterministic from the same
// list of kept reads); each allele is the voted consensus of a repaired group or the backbone of a group that needed none.
// (SNV forms: a locus of the SNV branch waits with FL_REPAIRED | FL_SNV; its assignment is read back from snv_read, its counts from pend
// and pend_hap)
template <int MAXR, bool PRESEL = false, bool SNV = false>
__global__ void __launch_bounds__(64) cluster_flank_finish_kernel(const ClFlankArgsOf<SNV> a) {
  __shared__ gt::FinShared<MAXR> sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const gt::GtArgs& g = a.c.g;
  const int64_t l = a.c.list[k];
  bool snv = false;
  if constexpr (SNV) snv = a.flank_done[l] == (gt::FL_REPAIRED | gt::FL_SNV);
  if (a.flank_done[l] != gt::FL_REPAIRED && !snv) return;
  const int lane = threadIdx.x;
  const uint64_t r0 = g.locus_read_begin[l];
  const int nr = (int)(g.locus_read_begin[l + 1] - r0);
  if (lane == 0) sh.n = 0;
  gt::gt_selected<MAXR, PRESEL>(sh, g, l, r0, nr, lane);
  const int n = sh.n;
  const ClFlankPend pd = a.pend[k];
  int cnt[2] = {0, 0};
  int32_t hap[2] = {0, 0};  // (SNV forms) the assigned reads of either group of a locus of the SNV branch
  bool fail;
  if (snv) {
    if constexpr (SNV) {
      for (int i = lane; i < n; i += 64) sh.cls[i] = (int8_t)(a.snv_read[r0 + i] & gt::SR_ASSIGN);
      hap[0] = a.pend_hap[2 * k]; hap[1] = a.pend_hap[2 * k + 1];
      __syncthreads();
    }
    fail = n == 0 || n != hap[0] + hap[1];
  } else fail = n == 0 || !gt::flank_assign(sh, a.hp_tag, r0, n, lane, cnt) || cnt[0] != pd.cnt[0] || cnt[1] != pd.cnt[1];
  const uint8_t mark = snv ? (uint8_t)gt::FL_SNV : (uint8_t)0;
  const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0};
  for (int q = 0; q < 2 && !fail; ++q) {
    if (pd.grp[q] >= 0) {
      const uint32_t voted = a.c.vote_len[pd.grp[q]];
      if (voted == 0xFFFFFFFFu) { fail = true; break; }  // the vote gave up on the group (overflow of its result slot)
      ap[q] = a.c.vote_out + a.c.groups[pd.grp[q]].out_off; aln[q] = voted;
    } else { ap[q] = g.reads + pd.bb_off[q]; aln[q] = pd.bb_len[q]; }
  }
  if (fail) { hand_back(a, l, lane, mark); return; }
  const uint8_t* const apc[2] = {ap[0], ap[1]};
  if (snv) flank_write(sh, a, l, r0, n, lane, apc, aln, pd.civ, hap, (uint8_t)(gt::FL_DONE | gt::FL_REPAIRED), mark);
  else flank_write(sh, a, l, r0, n, lane, apc, aln, pd.civ, pd.cnt, (uint8_t)(gt::FL_DONE | gt::FL_REPAIRED));
}

}  // namespace clf
}  // namespace trgt
