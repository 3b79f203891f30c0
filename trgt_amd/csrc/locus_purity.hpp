// trgt_amd/csrc/locus_purity.hpp -- filter_impure_trs (src/trgt/workflows/tr.rs:37-50, 400-452) between get_spanning_reads and the
// genotypers, for the calls with min_read_qual < 0.9 (MIN_RQ_FOR_PURITY), so that they keep the device-side genotyper chains:
//   purity_select_kernel  get_spanning_reads (gt_front, unchanged) for every locus of the genotypers' envelope; the kept reads go to
//                         global memory in LocusResult.reads order, and every kept read whose quality is not >= 0.9 (None = NaN
//                         included) becomes one purity job: its repeat segment under the locus's motif HMM
//   (the purity-only HMM batch over those jobs: hmm_batch_impl with spans3 == NULL, its purities left in HBM; locus.hip)
//   purity_filter_kernel  tr.rs:438-448: stable sort by f64::total_cmp of the purities (reads without a job: exactly 1.0), then the
//                         front-to-back walk that drops at most max(1, round(0.1 n)) reads below 0.9
// One wavefront per locus, like the genotypers.  The list the second kernel leaves behind is what the PRESEL instantiations of the
// genotyper kernels load instead of calling gt_front (gt_selected, locus_gt.hpp).
#pragma once
#include "locus_gt.hpp"

namespace trgt {
namespace pur {

constexpr uint32_t NO_JOB = 0xFFFFFFFFu;

struct PurityJob { uint64_t seq_off; uint32_t seq_len; uint32_t locus; };  // the repeat segment in the read blob; the motif set is the locus

struct PurityArgs {
  const double* read_qual;     // per read of the batch (NaN = None); nullptr: None for every read
  int32_t skip_cluster;        // 1: Genotyper::Cluster loci are genotyped by the host (which selects and filters them itself)
  uint32_t *sel_read, *sel_start, *sel_len;  // [reads of the batch] the kept reads of locus l in slots [locus_read_begin[l], + n_sel[l])
  uint32_t* n_sel;             // [n_loci]
  uint32_t* sel_job;           // [reads of the batch] per slot: the purity job of the read, NO_JOB = not scored (purity 1.0)
  uint32_t* counter;           // number of purity jobs (cleared before the launch)
  PurityJob* jobs;             // [cap_jobs] pinned host memory: the host builds the HMM batch from it
  uint32_t cap_jobs;           // the batch's read count: every read is kept at most once
  const double* purity;        // [cap_jobs] per job, as the HMM kernels wrote it (purity_filter_kernel)
};

__device__ __forceinline__ unsigned long long lanes_under(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// ---- 1. spanning reads of every locus the device genotypers take, and the purity jobs of the reads without a quality >= 0.9
template <int MAXR>
__global__ void __launch_bounds__(64) purity_select_kernel(const gt::GtArgs a, const PurityArgs p) {
  __shared__ gt::FinShared<MAXR> sh;
  __shared__ uint32_t s_base;
  const int64_t l = blockIdx.x;
  if (l >= a.n_loci) return;
  const int lane = threadIdx.x;
  const uint64_t r0 = a.locus_read_begin[l];
  const int nr = (int)(a.locus_read_begin[l + 1] - r0);
  if (lane == 0) { sh.n = 0; p.n_sel[l] = 0; }
  // the genotypers' envelope: the loci outside it are empty (Ploidy::Zero, no read) or take the host path with their need_host flag
  if (a.ploidy[l] == 0 || nr == 0 || nr > MAXR || (p.skip_cluster && a.genotyper && a.genotyper[l] == 1)) return;
  gt::gt_front<MAXR>(sh, a, r0, nr, lane);
  const int n = sh.n;
  // Some(rq) with rq >= cutoff keeps purity 1.0; None (NaN) and low qualities are scored: the comparison of the host path, so NaN falls through
  auto scored = [&](int i) { const double rq = p.read_qual ? p.read_qual[r0 + sh.s_read[i]] : __longlong_as_double(0x7FF8000000000000ll); return !(rq >= 0.9); };
  uint32_t cnt = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    cnt += (uint32_t)__popcll(__ballot(i < n && scored(i)));
  }
  if (lane == 0) s_base = cnt ? atomicAdd(p.counter, cnt) : 0u;
  __syncthreads();
  uint32_t at = s_base;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool job = i < n && scored(i);
    const unsigned long long mask = __ballot(job);
    if (i < n) {
      const uint32_t j = job ? at + (uint32_t)__popcll(mask & lanes_under(lane)) : NO_JOB;
      p.sel_read[r0 + i] = sh.s_read[i]; p.sel_start[r0 + i] = sh.s_start[i]; p.sel_len[r0 + i] = sh.s_len[i];
      p.sel_job[r0 + i] = j < p.cap_jobs ? j : NO_JOB;  // (j < cap_jobs always: a read is kept at most once)
      if (job && j < p.cap_jobs) { PurityJob pj; pj.seq_off = sh.r_off[sh.s_read[i]] + sh.s_start[i]; pj.seq_len = sh.s_len[i]; pj.locus = (uint32_t)l; p.jobs[j] = pj; }
    }
    at += (uint32_t)__popcll(mask);
  }
  if (lane == 0) p.n_sel[l] = (uint32_t)n;
}

// f64::total_cmp as a signed integer order on the bits (what the host path's total_key does)
__device__ __forceinline__ long long total_key(double d) {
  long long b = __double_as_longlong(d);
  b ^= (long long)((unsigned long long)(b >> 63) >> 1);
  return b;
}

// ---- 2. tr.rs:438-448 on the selected list of a locus, in place
template <int MAXR>
struct FilterShared {
  long long key[MAXR]; double pv[MAXR];
  uint32_t rd[MAXR], st[MAXR], ln[MAXR];
  int pos[MAXR];  // slot of the read after the walk, -1: dropped
  int m;
};
template <int MAXR>
__global__ void __launch_bounds__(64) purity_filter_kernel(const gt::GtArgs a, const PurityArgs p) {
  __shared__ FilterShared<MAXR> sh;
  const int64_t l = blockIdx.x;
  if (l >= a.n_loci) return;
  const int lane = threadIdx.x;
  const uint64_t r0 = a.locus_read_begin[l];
  const int n = min((int)p.n_sel[l], MAXR);  // (0 for the loci the selection left alone; never more than the locus has reads)
  if (n == 0) return;
  for (int i = lane; i < n; i += 64) {
    const uint32_t j = p.sel_job[r0 + i];
    sh.key[i] = total_key(j == NO_JOB ? 1.0 : p.purity[j]);
  }
  __syncthreads();
  {
    // ---- stable sort by purity: rank = #{smaller key} + #{equal key and earlier}; every lane owns elements lane, lane+64, ...
    uint32_t rd[MAXR / 64], st[MAXR / 64], ln[MAXR / 64]; long long ky[MAXR / 64]; int rk[MAXR / 64];
    for (int t = 0; t < MAXR / 64; ++t) {
      const int i = lane + 64 * t;
      rk[t] = -1;
      if (i < n) {
        rd[t] = p.sel_read[r0 + i]; st[t] = p.sel_start[r0 + i]; ln[t] = p.sel_len[r0 + i]; ky[t] = sh.key[i];
        int r = 0;
        for (int j = 0; j < n; ++j) { const long long kj = sh.key[j]; r += (kj < ky[t]) || (kj == ky[t] && j < i); }
        rk[t] = r;
      }
    }
    for (int t = 0; t < MAXR / 64; ++t)
      if (rk[t] >= 0) {
        const uint32_t j = p.sel_job[r0 + lane + 64 * t];
        sh.rd[rk[t]] = rd[t]; sh.st[rk[t]] = st[t]; sh.ln[rk[t]] = ln[t]; sh.pv[rk[t]] = j == NO_JOB ? 1.0 : p.purity[j];
      }
    __syncthreads();
  }
  if (lane == 0) {
    // ---- front to back: an impure read is dropped while the budget lasts (NaN is not >= 0.9: an empty repeat segment counts as impure)
    const size_t rounded = (size_t)round(0.1 * (double)n);  // f64, half away from zero: std::round of the host path
    const size_t max_filter = rounded > 1 ? rounded : 1;
    size_t filtered = 0; int m = 0;
    for (int i = 0; i < n; ++i) {
      if (sh.pv[i] >= 0.9 || filtered >= max_filter) sh.pos[i] = m++;
      else { sh.pos[i] = -1; ++filtered; }
    }
    sh.m = m;
  }
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const int q = sh.pos[i];
    if (q >= 0) { p.sel_read[r0 + q] = sh.rd[i]; p.sel_start[r0 + q] = sh.st[i]; p.sel_len[r0 + q] = sh.ln[i]; }
  }
  if (lane == 0) p.n_sel[l] = (uint32_t)sh.m;
}

}  // namespace pur
}  // namespace trgt
