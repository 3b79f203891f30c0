// trgt_amd/csrc/repair_queue.hpp -- the queue in front of a consensus repair (repair_consensus, consensus.rs:5-111), stated once for every
// genotyper that feeds one: the size and haplotype-tag routes of locus_gt.hpp / locus_gt_deep.hpp (RepairBufs, RC_* counters) and the
// two consensus rounds of locus_cluster_dev.hpp / locus_cluster_deep.hpp (ClArgs, CC_* counters), with the third round the tag route of
// locus_cluster_flank.hpp adds behind the one-wave cluster chain (the chain's arenas, counters of its own).  A vote group is a backbone and its
// members, all segments of the read blob; queueing one means
//   group_needs      what the group takes from the three arenas: CIGAR words, result bytes, vote scratch words
//   reserve_arenas   the reservation of a locus (at most two groups) by ONE thread, broadcast through a Reserved record in LDS
//   queue_group      the RGroup record and one alignment job per member, with running CIGAR offsets (the workgroup-prefix form for deep
//                    loci is gtd::queue_group_scan, next to the scans it uses; both write through put_group / put_job)
// and behind the alignments and the column voting (consensus_vote.hpp) repaired_allele reads a result back.  Whoever changes the vote
// scratch layout, the CIGAR slot size or the arena order changes it here; repair_check_kernel (locus.hip) reads the same lists.
#pragma once
#include "common.hpp"
#include "wfa_host.hpp"

namespace trgt {
namespace gt {

struct RGroup {  // = vote::Group (consensus_vote.hpp; the layouts are asserted equal in locus.hip)
  uint32_t job_first, n_members, bb_len, out_cap;
  uint64_t bb_off, out_off, scratch_off;
};
struct RepairPend {  // what the genotyper had decided for a locus that waits for its repaired alleles
  int32_t n_gt, n_pick; uint32_t size[2]; int32_t civ[4]; int32_t rep[2] /* rank of the pick */; int32_t grp[2] /* vote group, -1: the pick stands */;
};
enum { RC_GROUPS = 0, RC_JOBS = 1, RC_LOCI = 2, RC_FAILED = 3, RC_CIGAR = 4 /* u64 */, RC_OUT = 6 /* u64 */, RC_SCRATCH = 8 /* u64 */, RC_REFUSED = 10 /* alignment jobs of the chain the generic kernel refused (beyond its planned workspace) */,
       // loci that left a lane-parallel section of locus_genotype_kernel (locus_gt.hpp): kept list not sorted by length (downsampled) -- the
       // length histogram is built read by read; segments not staged, or a hash collision -- the sequence histogram inserts every read
       RC_GT_UNSORTED = 11, RC_GT_NOFIT = 12, RC_GT_COLLISION = 13, RC_WORDS = 16 };
struct RepairBufs {
  uint32_t* counts;  // [RC_WORDS]; nullptr: no device-side repair (every such locus takes the host path)
  RGroup* groups; JobDev* jobs; uint32_t* loci; RepairPend* pend;
  uint32_t cap_groups, cap_jobs, max_seg, vote_lds_pos;
  uint64_t cap_cigar, cap_out, cap_scratch;
};
struct FinishArgs { const uint8_t* vote_out; const uint32_t* vote_len; };

// What a vote group of nm members (mbytes bytes in all) around a backbone of bb bytes takes: one CIGAR slot of bb + len + 1 words per
// member; a result of at most one base per backbone position plus the insertions taken, each of which is a piece of some member, in a
// 16-aligned slot; three scratch words per member, and per backbone position where the vote's LDS (vote_lds_pos positions) is too small.
struct GroupNeeds { unsigned long long cig, out_need, scr_need; uint32_t out_cap; };
__device__ __forceinline__ GroupNeeds group_needs(uint32_t bb, uint32_t nm, unsigned long long mbytes, uint32_t vote_lds_pos) {
  GroupNeeds nd;
  nd.cig = (unsigned long long)nm * ((unsigned long long)bb + 1) + mbytes;
  nd.out_cap = (uint32_t)(bb + mbytes + 16);
  nd.out_need = ((unsigned long long)nd.out_cap + 15ull) & ~15ull;
  nd.scr_need = (bb + 1 <= vote_lds_pos + 1 ? 0ull : 3ull * ((unsigned long long)bb + 1)) + 3ull * nm;
  return nd;
}

// The reservation of a locus as its workgroup sees it (one thread writes it to LDS), and while the groups are written the next free
// place in every list.  g0 / j0: first vote group / alignment job; c0 / o0 / s0: CIGAR words, result bytes, scratch words.
struct Reserved { int ok; uint32_t g0, j0; unsigned long long c0, o0, s0; };
static_assert(sizeof(Reserved) == 40, "the six words every kernel's LDS held for it");

// One thread reserves the arena space of both groups of a locus (an absent group needs nothing): CIGAR, result, scratch, in this order,
// and no arena is touched after one that had no room.  Before any job or group slot is taken: a failed reservation must not leave holes
// in the job list.  It is not rolled back either -- what it took stays taken for the rest of the call.
__device__ __forceinline__ bool reserve_arenas(uint32_t* cigar, uint32_t* out, uint32_t* scratch, uint64_t cap_cigar, uint64_t cap_out, uint64_t cap_scratch,
                                               const GroupNeeds (&nd)[2], Reserved& r) {
  auto take = [](uint32_t* counter, unsigned long long need, unsigned long long cap, unsigned long long& base) {
    base = atomicAdd(reinterpret_cast<unsigned long long*>(counter), need);
    return base + need <= cap;
  };
  r.c0 = r.o0 = r.s0 = 0;
  r.ok = take(cigar, nd[0].cig + nd[1].cig, cap_cigar, r.c0) && take(out, nd[0].out_need + nd[1].out_need, cap_out, r.o0) &&
         take(scratch, nd[0].scr_need + nd[1].scr_need, cap_scratch, r.s0);
  return r.ok != 0;
}

// ... of a locus of the size or tag routes, by one thread: the arenas, its jobs and groups, and its place in the list of waiting loci
__device__ __forceinline__ void repair_reserve(const RepairBufs& rp, int64_t l, int64_t n_loci, uint32_t n_jobs, uint32_t n_groups, const GroupNeeds (&nd)[2], Reserved& r) {
  if (!reserve_arenas(rp.counts + RC_CIGAR, rp.counts + RC_OUT, rp.counts + RC_SCRATCH, rp.cap_cigar, rp.cap_out, rp.cap_scratch, nd, r)) { atomicAdd(rp.counts + RC_FAILED, 1u); return; }
  r.j0 = atomicAdd(rp.counts + RC_JOBS, n_jobs);
  r.g0 = atomicAdd(rp.counts + RC_GROUPS, n_groups);
  if (r.j0 + n_jobs > rp.cap_jobs || r.g0 + 2 > rp.cap_groups) r.ok = 0;  // (cannot happen: the caps are the read and locus counts)
  else { const uint32_t slot = atomicAdd(rp.counts + RC_LOCI, 1u); if (slot < (uint32_t)n_loci) rp.loci[slot] = (uint32_t)l; else r.ok = 0; }
}

struct Seg { unsigned long long off; uint32_t len; };  // a segment of the read blob
// the record of the group at `at` (one thread) / alignment job j of a group: member against backbone, CIGAR slot at cigar_off
__device__ __forceinline__ void put_group(RGroup* groups, const Reserved& at, Seg bb, uint32_t nm, const GroupNeeds& nd) {
  RGroup G;
  G.job_first = at.j0; G.n_members = nm; G.bb_len = bb.len; G.out_cap = nd.out_cap;
  G.bb_off = bb.off; G.out_off = at.o0; G.scratch_off = at.s0;
  groups[at.g0] = G;
}
__device__ __forceinline__ void put_job(JobDev* jobs, uint32_t j, Seg bb, Seg member, unsigned long long cigar_off) {
  JobDev jd;
  jd.pat_off = bb.off; jd.pat_len = bb.len;
  jd.txt_off = member.off; jd.txt_len = member.len;
  jd.cigar_off = cigar_off; jd.ops_off = 0; jd.out_index = j; jd.pad = 0;
  jobs[j] = jd;
}
// Queues one vote group at `at`, by a workgroup of W threads that all walk the n items: is_member(i) says whether item i belongs to the
// group, seg(i) is its segment; member k of the group becomes job at.j0 + k, written by thread k % W, with its CIGAR slot behind
// those of the members before it.  Moves `at` behind the group and returns the group's index.
template <int W, class IsMember, class SegOf>
__device__ __forceinline__ uint32_t queue_group(RGroup* groups, JobDev* jobs, Reserved& at, Seg bb, uint32_t nm, const GroupNeeds& nd, int n, IsMember is_member, SegOf seg) {
  const uint32_t g = at.g0;
  if (threadIdx.x == 0) put_group(groups, at, bb, nm, nd);
  uint32_t k = 0;
  for (int i = 0; i < n; ++i) {
    if (!is_member(i)) continue;
    if ((k & (uint32_t)(W - 1)) == threadIdx.x) put_job(jobs, at.j0 + k, bb, seg(i), at.c0);
    at.c0 += (unsigned long long)bb.len + seg(i).len + 1;
    ++k;
  }
  at.j0 += nm; at.o0 += nd.out_need; at.s0 += nd.scr_need; ++at.g0;
  return g;
}

// Allele al of a locus that waited: the repaired sequence of its vote group, or the pick / backbone that stood (seg(rank) is the segment
// of a kept read).  false: the vote gave up on the group (overflow of its result slot) and the locus takes the host path.
template <class SegOf>
__device__ __forceinline__ bool repaired_allele(const RepairPend& pd, int al, const FinishArgs& f, const RepairBufs& rp, const uint8_t* reads, SegOf seg, const uint8_t*& p, uint32_t& len) {
  if (pd.grp[al] >= 0) {
    const uint32_t voted = f.vote_len[pd.grp[al]];
    if (voted == 0xFFFFFFFFu) return false;  // (p and len stay as they were)
    p = f.vote_out + rp.groups[pd.grp[al]].out_off; len = voted;
  } else { const Seg s = seg(pd.rep[al]); p = reads + s.off; len = s.len; }
  return true;
}

}  // namespace gt
}  // namespace trgt
