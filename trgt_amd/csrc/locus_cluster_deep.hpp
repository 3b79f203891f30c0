// trgt_amd/csrc/locus_cluster_deep.hpp -- the deep instantiation of the device-side cluster genotyper: Genotyper::Cluster loci with more
// than gt::GT_MAX_READS (256) candidate reads, up to CL_DEEP_MAX_READS, for the contexts that opted in (trgt_hip_set_cluster_max_reads).
// The reference's --preset targeted (cli.rs:265-341: cluster genotyper, --max-depth 10000, --min-read-quality -1.0) is built around such
// loci; without this chain every one of them takes the host path of locus_cluster.hpp.
//
// Same stages, same launches in between and the same decisions as locus_cluster_dev.hpp (genotype_cluster.rs:58-152), which this file
// restates for one WORKGROUP of DW threads per locus instead of one wave:
//   deep_select_kernel    get_spanning_reads (tr.rs:111-184): filter, stable sort by span length, uniform downsample; the kept reads always
//                         go to global lists (what the PRESEL instantiations of the one-wave kernels load), so every later kernel has one
//                         way to find them whether filter_impure_trs is on or off; with the filter on, the purity jobs as well
//   deep_filter_kernel    tr.rs:438-448 on that list (behind the purity-only HMM batch of locus.hip, which is shared with the shallow loci)
//   deep_front_kernel     pair list / length differences (get_dist_matrix :250-286)           -> the score-only BiWFA launch
//   deep_linkage_kernel   Ward linkage, Muellner's NN-chain with in-place Lance-Williams updates; the merges go to global memory
//   deep_groups_kernel    stable sort of the merges, SciPy labels, cut-off, groups, backbones, consensus jobs (reserved and written by
//                         repair_queue.hpp, as in every chain) -> BiWFA launch + votes
//   deep_round2_kernel    small_group_is_outlier and the even / odd redo, dropped reads against both alleles -> second round
//   deep_finish_kernel    classifications, allele order, reference allele first, outputs
// The matrix lives in HBM (ClArgs::gmat); per-read state that the one-wave kernels keep in LDS structs is in LDS where a single thread
// walks it (labels, cut-off, groups: tens of KB at 2 048 reads) and in per-locus global lists otherwise.
// Ties: every "first minimum in index order" of the reference's sequential scans is a minimum over (value, index) pairs, compared
// lexicographically, first inside each thread (ascending indices, strict <), then across the wave and the workgroup: the smallest value
// and among equals the lowest index, whichever thread looked at it.  The f64 expressions are those of locus_cluster_dev.hpp, in its order.
// (The developer switches of tools/unpinned_sensitivity.py -- ClArgs::flags -- act on the one-wave kernels only.)
#pragma once
#include "locus_cluster_dev.hpp"
#include "locus_purity.hpp"

namespace trgt {
namespace cld {

constexpr int CL_DEEP_MAX_READS = 2048;  // reads of a locus the deep chain takes (README "Limits")
constexpr int DW = 256;                  // threads per locus: four waves
constexpr int DWAVES = DW / 64;
constexpr int DT = CL_DEEP_MAX_READS / DW;  // elements a thread holds in registers across a rank sort
static_assert(CL_DEEP_MAX_READS % DW == 0 && 2 * CL_DEEP_MAX_READS <= 32767, "labels of the dendrogram (up to 2 n - 2) are 16-bit");

struct DeepArgs {
  cl::ClArgs c;  // the deep list's own job lists, arenas, counters, records and matrix
  uint32_t *sel_read, *sel_start, *sel_len, *sel_job;  // [reads of the batch] kept reads of a locus at locus_read_begin + rank (sel_job: purity job, pur::NO_JOB = purity 1.0)
  uint32_t* n_sel;                                     // [n_list]
  uint16_t *mg_a, *mg_b; double* mg_d;                 // [reads of the batch] merges of the linkage in the order they were made, at locus_read_begin + merge
  int32_t purity_on;                                   // filter_impure_trs: the selection emits purity jobs
  const double* read_qual; uint32_t* pj_counter; pur::PurityJob* pj; uint32_t pj_cap; const double* purity;  // = pur::PurityArgs
};

struct Red { double v[DWAVES]; int i[DWAVES]; uint32_t u[DWAVES]; };

// minimum of (v, i) over the workgroup, lexicographic; every thread gets the result
__device__ __forceinline__ void block_min_vi(double& v, int& i, Red& r) {
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o); const int wi = __shfl_xor(i, o);
    if (w < v || (w == v && wi < i)) { v = w; i = wi; }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { r.v[wave] = v; r.i[wave] = i; }
  __syncthreads();
  v = r.v[0]; i = r.i[0];
  for (int w = 1; w < DWAVES; ++w) { const double wv = r.v[w]; const int wi = r.i[w]; if (wv < v || (wv == v && wi < i)) { v = wv; i = wi; } }
  __syncthreads();
}
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t x, Red& r) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  if ((threadIdx.x & 63) == 0) r.u[threadIdx.x >> 6] = x;
  __syncthreads();
  uint32_t s = 0;
  for (int w = 0; w < DWAVES; ++w) s += r.u[w];
  __syncthreads();
  return s;
}
// position of a flagged thread among the flagged threads of the workgroup, in thread order, and their number
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t& total, Red& r) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) r.u[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t before = 0; total = 0;
  for (int w = 0; w < DWAVES; ++w) { const uint32_t cw = r.u[w]; before += w < wave ? cw : 0u; total += cw; }
  __syncthreads();
  return before + (uint32_t)__popcll(mask & cl::lanes_below(lane));
}

// ---- 1. get_spanning_reads (gt_front of locus_gt.hpp for a workgroup), the global lists, purity jobs
struct DeepSel { uint32_t rd[CL_DEEP_MAX_READS], st[CL_DEEP_MAX_READS], ln[CL_DEEP_MAX_READS]; Red red; uint32_t base; };
__global__ void __launch_bounds__(DW) deep_select_kernel(const DeepArgs a) {
  __shared__ DeepSel sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const gt::GtArgs& g = a.c.g;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  const uint64_t r0 = g.locus_read_begin[l];
  const int nr = (int)(g.locus_read_begin[l + 1] - r0);
  if (g.ploidy[l] == 0 || nr == 0 || nr > CL_DEEP_MAX_READS) { if (tid == 0) a.n_sel[k] = 0; return; }
  const int F = g.flank_len;
  int n = 0;
  for (int base = 0; base < nr; base += DW) {  // filter of get_spanning_reads (tr.rs:139-145), kept in read order
    const int i = base + tid;
    int32_t s = 0, e = 0; bool keep = false;
    if (i < nr) { s = g.span_start[r0 + i]; e = g.span_end[r0 + i]; keep = s >= 0 && s >= F && (int64_t)g.read_len[r0 + i] - e >= F; }
    uint32_t total;
    const uint32_t pos = (uint32_t)n + block_rank(keep, total, sh.red);
    if (keep) { sh.rd[pos] = (uint32_t)i; sh.st[pos] = (uint32_t)s; sh.ln[pos] = (uint32_t)(e - s); }
    n += (int)total;
  }
  __syncthreads();
  if (n > 0) {
    // ---- stable sort by span length (:157): rank = #{shorter} + #{equal and earlier}; thread t owns elements t, t + DW, ...
    uint32_t rd[DT], st[DT], ln[DT]; int rk[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int i = tid + DW * t;
      rk[t] = 0; rd[t] = st[t] = 0; ln[t] = 0;
      if (i < n) { rd[t] = sh.rd[i]; st[t] = sh.st[i]; ln[t] = sh.ln[i]; }
    }
    for (int j = 0; j < n; ++j) {
      const uint32_t lj = sh.ln[j];
#pragma unroll
      for (int t = 0; t < DT; ++t) rk[t] += (lj < ln[t]) || (lj == ln[t] && j < tid + DW * t);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < DT; ++t)
      if (tid + DW * t < n) { sh.rd[rk[t]] = rd[t]; sh.st[rk[t]] = st[t]; sh.ln[rk[t]] = ln[t]; }
    __syncthreads();
    if (n > g.max_depth) {
      if (tid == 0) {  // ---- uniform downsample (:172-184), sequential swaps exactly as written there
        const double step = (double)n / (double)g.max_depth;
        double fast = 0.0;
        for (int i = 0; i < g.max_depth; ++i) {
          const int ind = (int)floor(fast);
          if (ind != i) {
            const uint32_t t0 = sh.rd[i], t1 = sh.st[i], t2 = sh.ln[i];
            sh.rd[i] = sh.rd[ind]; sh.st[i] = sh.st[ind]; sh.ln[i] = sh.ln[ind];
            sh.rd[ind] = t0; sh.st[ind] = t1; sh.ln[ind] = t2;
          }
          fast += step;
        }
      }
      n = g.max_depth;
      __syncthreads();
    }
  }
  if (a.purity_on) {
    // as purity_select_kernel: Some(rq) with rq >= 0.9 keeps purity 1.0; None (NaN) and low qualities are scored, in list order
    auto scored = [&](int i) { const double rq = a.read_qual ? a.read_qual[r0 + sh.rd[i]] : __longlong_as_double(0x7FF8000000000000ll); return !(rq >= 0.9); };
    uint32_t cnt = 0;
    for (int i = tid; i < n; i += DW) cnt += scored(i);
    cnt = block_sum_u32(cnt, sh.red);
    if (tid == 0) sh.base = cnt ? atomicAdd(a.pj_counter, cnt) : 0u;
    __syncthreads();
    uint32_t at = sh.base;
    for (int base = 0; base < n; base += DW) {
      const int i = base + tid;
      const bool job = i < n && scored(i);
      uint32_t total;
      const uint32_t j = at + block_rank(job, total, sh.red);
      if (i < n) {
        a.sel_job[r0 + i] = job && j < a.pj_cap ? j : pur::NO_JOB;  // (j < pj_cap always: a read is kept at most once)
        if (job && j < a.pj_cap) { pur::PurityJob pj; pj.seq_off = g.read_off[r0 + sh.rd[i]] + sh.st[i]; pj.seq_len = sh.ln[i]; pj.locus = (uint32_t)l; a.pj[j] = pj; }
      }
      at += total;
    }
  }
  for (int i = tid; i < n; i += DW) { a.sel_read[r0 + i] = sh.rd[i]; a.sel_start[r0 + i] = sh.st[i]; a.sel_len[r0 + i] = sh.ln[i]; }
  if (tid == 0) a.n_sel[k] = (uint32_t)n;
}

// ---- 1b. tr.rs:438-448 on the selected list of a locus, in place (purity_filter_kernel for a workgroup)
struct DeepFilt { long long key[CL_DEEP_MAX_READS]; uint32_t rd[CL_DEEP_MAX_READS], st[CL_DEEP_MAX_READS], ln[CL_DEEP_MAX_READS]; int16_t pos[CL_DEEP_MAX_READS]; int m; };
__global__ void __launch_bounds__(DW) deep_filter_kernel(const DeepArgs a) {
  __shared__ DeepFilt sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  const uint64_t r0 = a.c.g.locus_read_begin[l];
  const int n = min((int)a.n_sel[k], CL_DEEP_MAX_READS);
  if (n == 0) return;
  for (int i = tid; i < n; i += DW) {
    const uint32_t j = a.sel_job[r0 + i];
    sh.key[i] = pur::total_key(j == pur::NO_JOB ? 1.0 : a.purity[j]);
  }
  __syncthreads();
  {
    // ---- stable sort by f64::total_cmp of the purities: rank = #{smaller key} + #{equal key and earlier}
    uint32_t rd[DT], st[DT], ln[DT]; long long ky[DT]; int rk[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) {
      const int i = tid + DW * t;
      rk[t] = 0; rd[t] = st[t] = ln[t] = 0; ky[t] = 0;
      if (i < n) { rd[t] = a.sel_read[r0 + i]; st[t] = a.sel_start[r0 + i]; ln[t] = a.sel_len[r0 + i]; ky[t] = sh.key[i]; }
    }
    for (int j = 0; j < n; ++j) {
      const long long kj = sh.key[j];
#pragma unroll
      for (int t = 0; t < DT; ++t) rk[t] += (kj < ky[t]) || (kj == ky[t] && j < tid + DW * t);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < DT; ++t)
      if (tid + DW * t < n) { sh.rd[rk[t]] = rd[t]; sh.st[rk[t]] = st[t]; sh.ln[rk[t]] = ln[t]; sh.key[rk[t]] = ky[t]; }
    __syncthreads();
  }
  if (tid == 0) {
    // ---- front to back: an impure read is dropped while the budget lasts (NaN is not >= 0.9)
    const size_t rounded = (size_t)round(0.1 * (double)n);
    const size_t max_filter = rounded > 1 ? rounded : 1;
    size_t filtered = 0; int m = 0;
    for (int i = 0; i < n; ++i) {
      long long b = sh.key[i];  // (total_key is its own inverse)
      b ^= (long long)((unsigned long long)(b >> 63) >> 1);
      const double pv = __longlong_as_double(b);
      if (pv >= 0.9 || filtered >= max_filter) sh.pos[i] = (int16_t)m++;
      else { sh.pos[i] = -1; ++filtered; }
    }
    sh.m = m;
  }
  __syncthreads();
  for (int i = tid; i < n; i += DW) {
    const int q = sh.pos[i];
    if (q >= 0) { a.sel_read[r0 + q] = sh.rd[i]; a.sel_start[r0 + q] = sh.st[i]; a.sel_len[r0 + q] = sh.ln[i]; }
  }
  if (tid == 0) a.n_sel[k] = (uint32_t)sh.m;
}

__device__ __forceinline__ uint64_t seg_off(const DeepArgs& a, uint64_t r0, int i) { return a.c.g.read_off[r0 + a.sel_read[r0 + i]] + a.sel_start[r0 + i]; }

// ---- 2. pair list (the order of the jobs inside the list decides nothing: every job names its own slot)
struct DeepFront { uint32_t ln[CL_DEEP_MAX_READS]; uint64_t off[CL_DEEP_MAX_READS]; Red red; uint32_t base, cursor; };
__global__ void __launch_bounds__(DW) deep_front_kernel(const DeepArgs a) {
  __shared__ DeepFront sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t r0 = a.c.g.locus_read_begin[l];
  const int nr = (int)(a.c.g.locus_read_begin[l + 1] - r0);
  const int n = min((int)a.n_sel[k], min(nr, CL_DEEP_MAX_READS));
  cl::ClRec rec;
  rec.n = n; rec.state = n > 0 ? 1 : 0; rec.n_groups = 0; rec.redo = 0;
  for (int q = 0; q < 2; ++q) { rec.grp[q] = -1; rec.gsize[q] = 0; rec.cr_eo[q] = 0; }
  for (int q = 0; q < 4; ++q) { rec.ci[q] = 0; rec.ci_eo[q] = 0; }
  if (tid == 0) a.c.rec[k] = rec;
  if (n < 3) return;  // (no decision reads the matrix of one or two sequences)
  for (int i = tid; i < n; i += DW) { sh.ln[i] = a.sel_len[r0 + i]; sh.off[i] = seg_off(a, r0, i); }
  __syncthreads();
  uint32_t cnt = 0;
  for (int i = wave; i + 1 < n; i += DWAVES) {
    const uint64_t li = sh.ln[i];
    for (int j = i + 1 + lane; j < n; j += 64) cnt += li * (uint64_t)sh.ln[j] <= cl::CL_MAX_OPS;
  }
  cnt = block_sum_u32(cnt, sh.red);
  if (tid == 0) { sh.base = atomicAdd(a.c.counts + cl::CC_ED, cnt); sh.cursor = 0; }
  __syncthreads();
  const uint32_t base = sh.base;
  const uint64_t m0 = a.c.mat_off[k];
  for (int i = wave; i + 1 < n; i += DWAVES) {  // a wave per row; the waves take their places in the list from a shared cursor
    const uint32_t li = sh.ln[i];
    const uint64_t oi = sh.off[i];
    for (int jb = i + 1; jb < n; jb += 64) {
      const int j = jb + lane;
      const bool valid = j < n;
      const uint32_t lj = valid ? sh.ln[j] : 0u;
      const bool job = valid && (uint64_t)li * (uint64_t)lj <= cl::CL_MAX_OPS;
      const unsigned long long mask = __ballot(job);
      uint32_t wb = 0;
      if (mask) { if (lane == 0) wb = atomicAdd(&sh.cursor, (uint32_t)__popcll(mask)); wb = __shfl(wb, 0); }
      if (valid) {
        const uint64_t slot = m0 + cl::pair_idx((uint32_t)n, (uint32_t)i, (uint32_t)j);
        if (job) {
          JobDev jd;
          jd.pat_off = oi; jd.pat_len = li; jd.txt_off = sh.off[j]; jd.txt_len = lj;
          jd.cigar_off = 0; jd.ops_off = 0; jd.out_index = (uint32_t)slot; jd.pad = 0;
          a.c.ed_jobs[base + wb + (uint32_t)__popcll(mask & cl::lanes_below(lane))] = jd;
        } else a.c.escore[slot] = (int32_t)(li > lj ? li - lj : lj - li);
      }
    }
  }
}

// ---- 3. the matrix and the linkage (ward_nnchain of locus_cluster.hpp, operation for operation)
struct DeepLink { uint8_t act[CL_DEEP_MAX_READS]; uint16_t mem[CL_DEEP_MAX_READS]; int16_t chain[CL_DEEP_MAX_READS + 4]; Red red; };
__global__ void __launch_bounds__(DW) deep_linkage_kernel(const DeepArgs a) {
  __shared__ DeepLink sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const cl::ClRec rec = a.c.rec[k];
  if (rec.state != 1 || rec.n < 3) return;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  const uint64_t r0 = a.c.g.locus_read_begin[l];
  const int n = rec.n;
  const uint32_t un = (uint32_t)n;
  const bool one_group = a.c.g.ploidy[l] == 1;
  const uint64_t m0 = a.c.mat_off[k];
  double* const D = a.c.gmat + m0;
  const uint32_t np = un * (un - 1) / 2;
  // sqrt(score as f64) (get_dist :247); kodama squares it in place (linkage, Method::Ward)
  for (uint32_t p = (uint32_t)tid; p < np; p += DW) {
    const double d = __builtin_sqrt((double)a.c.escore[m0 + p]);
    D[p] = one_group ? d : d * d;
  }
  if (one_group) return;
  for (int i = tid; i < n; i += DW) { sh.act[i] = 1; sh.mem[i] = 1; }
  __syncthreads();
  const double inf = __builtin_huge_val();
  constexpr int NONE = 0x7FFFFFFF;
  // smallest D(i, cur) over the active i != cur, and the smallest such i among equals
  auto scan = [&](int cur, double& vmin, int& imin) {
    double bv = inf; int bi = NONE;
    for (int i = tid; i < n; i += DW)
      if (i != cur && sh.act[i]) { const double v = D[cl::pair_sym(un, (uint32_t)i, (uint32_t)cur)]; if (v < bv) { bv = v; bi = i; } }
    block_min_vi(bv, bi, sh.red);
    vmin = bv; imin = bi == NONE ? -1 : bi;
  };
  int chain_len = 0;
  for (int merge = 0; merge + 1 < n; ++merge) {
    int tip, nearest; double best;
    if (chain_len <= 3) {
      double z = 0.0; int h = NONE;
      for (int i = tid; i < n; i += DW) if (sh.act[i]) { h = i; break; }
      block_min_vi(z, h, sh.red);  // the first active element
      tip = h;
      sh.chain[0] = (int16_t)tip; chain_len = 1;
      scan(tip, best, nearest);
    } else {
      nearest = sh.chain[chain_len - 3];  // the merged pair and the element before it leave the chain; that element is looked at again
      chain_len -= 3;
      tip = sh.chain[chain_len - 1];
      best = D[cl::pair_sym(un, (uint32_t)tip, (uint32_t)nearest)];
    }
    for (;;) {  // until two clusters are each other's nearest neighbour; ties keep the previous chain element
      const int cur = nearest;
      sh.chain[chain_len++] = (int16_t)cur;  // (every thread writes the same value; the barriers of scan order it before the reads)
      double vmin; int imin;
      scan(cur, vmin, imin);
      int nn = tip;
      if (imin >= 0 && vmin < best) { best = vmin; nn = imin; }
      tip = cur; nearest = nn;
      if (nearest == sh.chain[chain_len - 2]) break;
    }
    const int lo = tip < nearest ? tip : nearest, hi = tip < nearest ? nearest : tip;
    const double s_lo = (double)sh.mem[lo], s_hi = (double)sh.mem[hi];
    for (int x = tid; x < n; x += DW) {  // Lance-Williams, written into the rows of the larger index; a thread touches its own x only
      if (x != lo && x != hi && sh.act[x]) {
        const double sx = (double)sh.mem[x];
        const double d_lo = D[cl::pair_sym(un, (uint32_t)x, (uint32_t)lo)];
        double* const ph = D + cl::pair_sym(un, (uint32_t)x, (uint32_t)hi);
        const double d_hi = *ph;
        *ph = (((sx + s_lo) * d_lo) + ((sx + s_hi) * d_hi) - (sx * best)) / (s_lo + s_hi + sx);
      }
    }
    __syncthreads();
    if (tid == 0) {
      sh.mem[hi] = (uint16_t)(sh.mem[hi] + sh.mem[lo]); sh.act[lo] = 0;
      a.mg_a[r0 + merge] = (uint16_t)lo; a.mg_b[r0 + merge] = (uint16_t)hi; a.mg_d[r0 + merge] = best;
    }
    __syncthreads();
  }
}

// ---- 4. groups, backbones, consensus jobs
struct DeepGroups {
  uint16_t so_a[CL_DEEP_MAX_READS], so_b[CL_DEEP_MAX_READS], so_size[CL_DEEP_MAX_READS]; double so_d[CL_DEEP_MAX_READS];  // merges sorted and relabelled (so_d: later the group sizes)
  alignas(8) uint8_t x[8 * CL_DEEP_MAX_READS];  // first the dissimilarities in merge order (f64), then up / member (int16 [2 n] each)
  uint16_t gm[CL_DEEP_MAX_READS];
  int8_t cls[CL_DEEP_MAX_READS];
  uint32_t ln[CL_DEEP_MAX_READS];
  Red red;
  gt::Reserved rsv;  // (ok: also the size of the group at hand)
};
// central_read (:12-39) as central_read_wave: every member's sum in the reference's order, the first minimum over the members
__device__ __forceinline__ int central_read_block(const double* D, uint32_t n, const uint16_t* gm, int cnt, Red& red) {
  if (cnt <= 2) return gm[0];
  constexpr int NONE = 0x7FFFFFFF;
  double best_v = __builtin_huge_val(); int best_m = NONE;
  for (int m = threadIdx.x; m < cnt; m += DW) {
    const uint32_t gmm = gm[m];
    double sum = 0.0;
    for (int q = 0; q < cnt; ++q) {
      if (q == m) continue;
      const uint32_t gq = gm[q];
      sum += D[q < m ? cl::pair_idx(n, gq, gmm) : cl::pair_idx(n, gmm, gq)];
    }
    if (best_m == NONE || sum < best_v) { best_v = sum; best_m = m; }
  }
  block_min_vi(best_v, best_m, red);
  return gm[best_m == NONE ? 0 : best_m];
}
__global__ void __launch_bounds__(DW) deep_groups_kernel(const DeepArgs a) {
  __shared__ DeepGroups sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  cl::ClRec rec = a.c.rec[k];
  if (rec.state != 1) return;
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  const uint64_t r0 = a.c.g.locus_read_begin[l];
  const int n = rec.n;
  const uint32_t un = (uint32_t)n;
  const int ploidy = a.c.g.ploidy[l] == 1 ? 1 : 2;
  const double* const D = a.c.gmat + a.c.mat_off[k];
  const bool one_group = ploidy == 1 || n == 1;
  double* const st_d = reinterpret_cast<double*>(sh.x);
  int16_t* const up = reinterpret_cast<int16_t*>(sh.x);
  int16_t* const member = up + 2 * CL_DEEP_MAX_READS;
  for (int i = tid; i < n; i += DW) { sh.cls[i] = 0; sh.ln[i] = a.sel_len[r0 + i]; }
  __syncthreads();
  int n_groups = 1;
  if (!one_group) {
    n_groups = 2;
    if (n == 2) {  // cluster(): [[0], [1]]; the stable sort by size keeps that order, the LAST group is popped first
      if (tid == 0) { sh.cls[0] = 1; sh.cls[1] = 0; }
    } else {
      // ---- stable sort of the merges by dissimilarity
      const int ns = n - 1;
      for (int s = tid; s < ns; s += DW) st_d[s] = a.mg_d[r0 + s];
      __syncthreads();
      for (int s = tid; s < ns; s += DW) {
        const double ds = st_d[s];
        int rk = 0;
        for (int j = 0; j < ns; ++j) { const double dj = st_d[j]; rk += (dj < ds) || (dj == ds && j < s); }
        sh.so_a[rk] = a.mg_a[r0 + s]; sh.so_b[rk] = a.mg_b[r0 + s]; sh.so_d[rk] = ds;
      }
      __syncthreads();
      for (int i = tid; i < 2 * n - 1; i += DW) { up[i] = -1; member[i] = -1; }
      __syncthreads();
      if (tid == 0) {
        // ---- SciPy labels: the clusters of a merge are named by their roots, the smaller label first
        for (int i = 0; i < ns; ++i) {
          int p = sh.so_a[i], q = sh.so_b[i];
          while (up[p] >= 0) p = up[p];
          while (up[q] >= 0) q = up[q];
          if (p > q) { const int w = p; p = q; q = w; }
          const int sp = p < n ? 1 : sh.so_size[p - n], sq = q < n ? 1 : sh.so_size[q - n];
          sh.so_a[i] = (uint16_t)p; sh.so_b[i] = (uint16_t)q; sh.so_size[i] = (uint16_t)(sp + sq);
          up[p] = up[q] = (int16_t)(n + i);
        }
        for (int i = 0; i < ns; ++i) sh.so_d[i] = __builtin_sqrt(sh.so_d[i]);
        // ---- cluster() (:154-227): the cut-off below the last merge of two clusters of at least min_cluster reads
        auto csize = [&](int label) { return label < n ? 1 : (int)sh.so_size[label - n]; };
        const double mc = __builtin_round(0.01 * (double)n);
        const int min_cluster = mc > 2.0 ? (int)mc : 2;
        double cutoff = 0.0;
        for (int i = ns - 1; i >= 0; --i) {
          const int ca = csize(sh.so_a[i]), cb = csize(sh.so_b[i]);
          if ((ca < cb ? ca : cb) >= min_cluster) { cutoff = sh.so_d[i] - 0.0001; break; }
        }
        int ng = 0;
        if (cutoff == 0.0) {  // homozygous: the reads are split evenly
          for (int i = 0; i < n; ++i) member[i] = (int16_t)(i & 1);
          ng = 2;
        } else {
          for (int i = ns - 1; i >= 0; --i) {
            if (!(sh.so_d[i] <= cutoff)) continue;
            int mine = member[n + i];
            if (mine < 0) { mine = ng++; member[n + i] = (int16_t)mine; }
            member[sh.so_a[i]] = (int16_t)mine; member[sh.so_b[i]] = (int16_t)mine;
          }
          for (int i = 0; i < n; ++i) if (member[i] < 0) member[i] = (int16_t)ng++;
        }
        // ---- the two largest groups; sort_by_key(len) is stable and pop() takes from the end: among equals the later group first
        uint16_t* const gsz = reinterpret_cast<uint16_t*>(sh.so_d);  // (the dissimilarities are not read again)
        for (int g = 0; g < ng; ++g) gsz[g] = 0;
        for (int i = 0; i < n; ++i) gsz[member[i]] += 1;
        int g0 = 0;
        for (int g = 1; g < ng; ++g) if (gsz[g] >= gsz[g0]) g0 = g;
        int g1 = -1;
        for (int g = 0; g < ng; ++g) if (g != g0 && (g1 < 0 || gsz[g] >= gsz[g1])) g1 = g;
        for (int i = 0; i < n; ++i) sh.cls[i] = (int8_t)(member[i] == g0 ? 0 : (member[i] == g1 ? 1 : 2));
      }
    }
    __syncthreads();
  }
  // ---- backbones (central_read on the matrix as it is now), intervals, jobs
  int bb[2] = {0, 0}, gcnt[2] = {0, 0};
  uint32_t ci[4] = {0, 0, 0, 0};
  unsigned long long mbytes[2] = {0, 0};
  for (int g = 0; g < n_groups; ++g) {
    __syncthreads();
    if (tid == 0) { int c = 0; for (int i = 0; i < n; ++i) if (sh.cls[i] == g) sh.gm[c++] = (uint16_t)i; sh.rsv.ok = c; }
    __syncthreads();
    gcnt[g] = sh.rsv.ok;
    bb[g] = central_read_block(D, un, sh.gm, gcnt[g], sh.red);
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (int q = 0; q < gcnt[g]; ++q) { const uint32_t ln = sh.ln[sh.gm[q]]; lo = ln < lo ? ln : lo; hi = ln > hi ? ln : hi; mbytes[g] += ln; }
    ci[2 * g] = lo; ci[2 * g + 1] = hi;
  }
  if (!one_group && n >= 3) {  // the even / odd split, should round 2 ask for it
    for (int g = 0; g < 2; ++g) {
      __syncthreads();
      if (tid == 0) { int c = 0; for (int i = g; i < n; i += 2) sh.gm[c++] = (uint16_t)i; sh.rsv.ok = c; }
      __syncthreads();
      rec.cr_eo[g] = central_read_block(D, un, sh.gm, sh.rsv.ok, sh.red);
      uint32_t lo = 0xFFFFFFFFu, hi = 0;
      for (int i = g; i < n; i += 2) { const uint32_t ln = sh.ln[i]; lo = ln < lo ? ln : lo; hi = ln > hi ? ln : hi; }
      rec.ci_eo[2 * g] = lo; rec.ci_eo[2 * g + 1] = hi;
    }
  }
  gt::GroupNeeds nd[2] = {};
#pragma unroll
  for (int g = 0; g < 2; ++g) if (g < n_groups) nd[g] = gt::group_needs(sh.ln[bb[g]], (uint32_t)gcnt[g], mbytes[g], a.c.vote_lds_pos);
  __syncthreads();
  if (tid == 0) cl::cluster_reserve(a.c, false, (uint32_t)(gcnt[0] + gcnt[1]), (uint32_t)n_groups, nd, sh.rsv);
  __syncthreads();
  if (!sh.rsv.ok) { rec.state = -1; if (tid == 0) a.c.rec[k] = rec; return; }
  gt::Reserved at = sh.rsv;
  auto seg_of = [&](int i) { return gt::Seg{seg_off(a, r0, i), sh.ln[i]}; };
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    if (g >= n_groups) break;
    rec.grp[g] = (int32_t)gt::queue_group<DW>(a.c.groups, a.c.jobs, at, seg_of(bb[g]), (uint32_t)gcnt[g], nd[g], n, [&, g](int i) { return sh.cls[i] == g; }, seg_of);
    rec.gsize[g] = gcnt[g];
  }
  rec.n_groups = n_groups;
  for (int q = 0; q < 4; ++q) rec.ci[q] = ci[q];
  if (tid == 0) a.c.rec[k] = rec;
  for (int i = tid; i < n; i += DW) a.c.cls[r0 + i] = sh.cls[i];
}

// ---- 5. behind the first consensus round: the homozygous redo, or the dropped reads against both alleles
struct DeepRound2 { uint32_t ln[CL_DEEP_MAX_READS]; gt::Reserved rsv; };
__global__ void __launch_bounds__(DW) deep_round2_kernel(const DeepArgs a) {
  __shared__ DeepRound2 sh;
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  cl::ClRec rec = a.c.rec[k];
  if (rec.state != 1) return;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int g = 0; g < rec.n_groups; ++g)
    if (a.c.vote_len[rec.grp[g]] == 0xFFFFFFFFu) { rec.state = -1; if (tid == 0) { a.c.rec[k] = rec; atomicAdd(a.c.counts + cl::CC_FAILED, 1u); } return; }
  if (rec.n_groups != 2) return;
  const int64_t l = a.c.list[k];
  const uint64_t r0 = a.c.g.locus_read_begin[l];
  const int n = rec.n;
  for (int i = tid; i < n; i += DW) sh.ln[i] = a.sel_len[r0 + i];
  __syncthreads();
  const uint32_t l1 = a.c.vote_len[rec.grp[0]], l2 = a.c.vote_len[rec.grp[1]];
  const uint32_t c1 = (uint32_t)rec.gsize[0], c2 = (uint32_t)rec.gsize[1];
  const uint32_t cmin = c1 < c2 ? c1 : c2, cmax = c1 < c2 ? c2 : c1;
  if ((l1 > l2 ? l1 - l2 : l2 - l1) < 100u && cmin * 4u < cmax) {  // small_group_is_outlier (:84-98): redo the homozygous case
    int gcnt[2] = {(n + 1) / 2, n / 2};
    unsigned long long mbytes[2] = {0, 0};
    for (int i = 0; i < n; ++i) mbytes[i & 1] += sh.ln[i];
    gt::GroupNeeds nd[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) nd[g] = gt::group_needs(sh.ln[rec.cr_eo[g]], (uint32_t)gcnt[g], mbytes[g], a.c.vote_lds_pos);
    if (tid == 0) cl::cluster_reserve(a.c, true, (uint32_t)n, 2u, nd, sh.rsv);
    __syncthreads();
    if (!sh.rsv.ok) { rec.state = -1; if (tid == 0) a.c.rec[k] = rec; return; }
    gt::Reserved at = sh.rsv;
    auto seg_of = [&](int i) { return gt::Seg{seg_off(a, r0, i), sh.ln[i]}; };
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      rec.grp[g] = (int32_t)gt::queue_group<DW>(a.c.groups, a.c.jobs, at, seg_of(rec.cr_eo[g]), (uint32_t)gcnt[g], nd[g], n, [g](int i) { return (i & 1) == g; }, seg_of);
      rec.gsize[g] = gcnt[g];
    }
    rec.redo = 1;
    for (int q = 0; q < 4; ++q) rec.ci[q] = rec.ci_eo[q];
    if (tid == 0) a.c.rec[k] = rec;
    return;
  }
  // the reads cluster() dropped go to the closer consensus (:117-142): their edit distances to both alleles (a wave takes its places in
  // the list by itself: the order of these jobs decides nothing either)
  const uint64_t aoff[2] = {a.c.groups[rec.grp[0]].out_off, a.c.groups[rec.grp[1]].out_off};
  const uint32_t alen[2] = {l1, l2};
  for (int ib = 0; ib < n; ib += DW) {
    const int i = ib + tid;
    const bool out = i < n && a.c.cls[r0 + i] == 2;
    const uint32_t li = i < n ? sh.ln[i] : 0u;
    uint32_t want = 0;
    if (out) for (int q = 0; q < 2; ++q) want += (uint64_t)li * (uint64_t)alen[q] <= cl::CL_MAX_OPS;
    uint32_t inc = want;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    const uint32_t total = __shfl(inc, 63);
    uint32_t base = 0;
    if (total) { if (lane == 0) base = atomicAdd(a.c.counts + cl::CC_ED2, total); base = __shfl(base, 0); }
    if (out) {
      uint32_t at = base + inc - want;
      for (int q = 0; q < 2; ++q) {
        const uint64_t slot = 2 * (r0 + (uint64_t)i) + (uint64_t)q;
        if ((uint64_t)li * (uint64_t)alen[q] <= cl::CL_MAX_OPS) {
          JobDev jd;
          jd.pat_off = seg_off(a, r0, i); jd.pat_len = li;
          jd.txt_off = aoff[q]; jd.txt_len = alen[q];
          jd.cigar_off = 0; jd.ops_off = 0; jd.out_index = (uint32_t)slot; jd.pad = 0;
          a.c.ed2_jobs[at++] = jd;
        } else a.c.escore2[slot] = (int32_t)(li > alen[q] ? li - alen[q] : alen[q] - li);
      }
    }
  }
}

// ---- 6. genotype, classifications, allele order (:143-151, :99-115, :62-73), reference allele first (tr.rs:95-101), outputs
__global__ void __launch_bounds__(DW) deep_finish_kernel(const DeepArgs a) {
  __shared__ int8_t s_cls[CL_DEEP_MAX_READS];
  const uint32_t k = blockIdx.x;
  if (k >= a.c.n_list) return;
  const gt::GtArgs& g = a.c.g;
  const cl::ClRec rec = a.c.rec[k];
  const int64_t l = a.c.list[k];
  const int tid = threadIdx.x;
  if (rec.state == 0) { if (tid == 0 && g.ploidy[l] != 0 && g.locus_read_begin[l + 1] != g.locus_read_begin[l]) g.need_host[l] = 0; return; }  // no spanning read: the empty result stands
  if (rec.state != 1) return;
  for (int q = 0; q < rec.n_groups; ++q)
    if (a.c.vote_len[rec.grp[q]] == 0xFFFFFFFFu) { if (tid == 0) atomicAdd(a.c.counts + cl::CC_FAILED, 1u); return; }
  const uint64_t r0 = g.locus_read_begin[l];
  const int n = rec.n;
  const int ploidy = g.ploidy[l] == 1 ? 1 : 2;
  const uint8_t* ap[2] = {nullptr, nullptr}; uint32_t aln[2] = {0, 0}; uint32_t civ[4] = {0, 0, 0, 0};
  for (int q = 0; q < rec.n_groups; ++q) {
    ap[q] = a.c.vote_out + a.c.groups[rec.grp[q]].out_off; aln[q] = a.c.vote_len[rec.grp[q]];
    civ[2 * q] = rec.ci[2 * q]; civ[2 * q + 1] = rec.ci[2 * q + 1];
  }
  int n_gt;
  for (int i = tid; i < n; i += DW) {
    int cc = 0;
    if (rec.n_groups == 2) {
      if (rec.redo) cc = i & 1;
      else {
        cc = a.c.cls[r0 + i];
        if (cc == 2) {  // tie_breaker starts at 1 for every read (:125): an exact tie resolves to (1 + 1) % 2 = 0
          const int32_t d1 = a.c.escore2[2 * (r0 + (uint64_t)i)], d2 = a.c.escore2[2 * (r0 + (uint64_t)i) + 1];
          cc = d1 < d2 ? 0 : (d2 < d1 ? 1 : 0);
        }
      }
    }
    s_cls[i] = (int8_t)cc;
  }
  __syncthreads();
  bool swapped = false;
  if (rec.n_groups == 1) {
    if (ploidy == 1) n_gt = 1;
    else { n_gt = 2; ap[1] = ap[0]; aln[1] = aln[0]; civ[2] = civ[0]; civ[3] = civ[1]; }  // one read, two alleles (:70-72)
  } else {
    n_gt = 2;
    if (aln[0] > aln[1]) {
      swapped = true;
      const uint8_t* tp = ap[0]; ap[0] = ap[1]; ap[1] = tp;
      const uint32_t tl = aln[0]; aln[0] = aln[1]; aln[1] = tl;
      uint32_t t0 = civ[0]; civ[0] = civ[2]; civ[2] = t0; t0 = civ[1]; civ[1] = civ[3]; civ[3] = t0;
    }
  }
  int by_hap[2] = {0, 0};
  for (int i = 0; i < n; ++i) { const int cc = swapped ? 1 - s_cls[i] : s_cls[i]; by_hap[cc] += 1; }
  const uint8_t* ref = g.tr_blob + g.tr_off[l]; const uint32_t refn = g.tr_len[l];
  int order[2] = {0, 1}, flip = 0;  // (wave_equal: every wave compares the whole strings, all reach the same answer)
  if (n_gt != 1 && !gt::wave_equal(ap[0], aln[0], ref, refn) && gt::wave_equal(ap[1], aln[1], ref, refn)) { order[0] = 1; order[1] = 0; flip = 1; }
  for (int oi = 0; oi < n_gt; ++oi) if (aln[order[oi]] > g.allele_cap[l]) { if (tid == 0) atomicAdd(a.c.counts + cl::CC_FAILED, 1u); return; }  // the host path reports the error
  for (int oi = 0; oi < n_gt; ++oi) {
    const int al = order[oi];
    uint8_t* dst = g.allele_blob + g.allele_off[2 * l + oi];
    for (uint32_t b = tid; b < aln[al]; b += DW) dst[b] = ap[al][b];
    if (tid == 0) {
      g.allele_len[2 * l + oi] = aln[al];
      g.ci[4 * l + 2 * oi] = (int32_t)civ[2 * al]; g.ci[4 * l + 2 * oi + 1] = (int32_t)civ[2 * al + 1];
      g.num_spanning[2 * l + oi] = by_hap[al];
      if (g.gt_size) g.gt_size[2 * l + oi] = (int32_t)aln[al];  // the cluster genotyper's sizes are its allele lengths
    }
  }
  for (int i = tid; i < n; i += DW) {
    const int cc = swapped ? 1 - s_cls[i] : s_cls[i];
    const uint32_t rd = a.sel_read[r0 + i];
    g.classification[r0 + rd] = flip ? 1 - cc : cc;
    g.read_rank[r0 + rd] = i;
  }
  if (tid == 0) {
    g.n_alleles[l] = n_gt; g.n_spanning_reads[l] = (uint32_t)n; g.flipped[l] = (uint8_t)flip; g.need_host[l] = 0;
    atomicAdd(a.c.counts + cl::CC_DONE, 1u);
  }
}

}  // namespace cld
}  // namespace trgt
