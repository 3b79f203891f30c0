// trgt_amd/csrc/locus_meth.hip -- trgt_locus_meth_batch: Allele::meth for the loci of a finished trgt_locus_batch call.
//
// Reference (PacificBiosciences/trgt v3.0.0, src/trgt/workflows/tr.rs):
//   get_meth      :198-230   per allele, the mean of the levels of the reads assign_read gives it, summed in LocusResult.reads order
//   assign_read   :239-266   First / Second / Both / None from the genotype's sizes and intervals, before "reference allele first"
//   get_tr_meth   :363-398   per read, the mean of meth[cpg_index] / 255 over the CpGs whose C lies inside the repeat span
//
// Two kernels, both one wave per item, both exact: every f64 sum is advanced in the reference's order by all lanes alike.
//   tr_meth_kernel      one wave per kept read.  The wave streams the read's bases up to the end of its span as aligned dwords (four ASCII
//                       bases or eight 4-bit codes per lane), marks the CpGs, counts the ones in front of the span and sums the calls of
//                       the ones inside it.  Level and span length go to the read's rank inside its locus.
//   allele_meth_kernel  one wave per locus.  It walks the ranks 64 at a time, evaluates assign_read per lane and advances the two sums.
#include "common.hpp"

#include <cmath>

namespace trgt {
namespace meth {

struct Job {           // one kept read (read_rank >= 0)
  uint64_t base_off;   // first byte of the read in the device blob
  uint64_t meth_off;   // first call of the read
  uint32_t read;       // input index (the malformed flag, read_meth)
  uint32_t len;        // bases
  int32_t s0, s1;      // the repeat span, 0 <= s0 <= s1 <= len
  uint32_t n_meth;     // calls of the read; 0: the read has none (has_meth 0 or an empty range) and gives no level
  uint32_t slot;       // locus_read_begin[l] + rank
};
struct Locus {         // the genotype in its OWN order (un-flipped), as assign_read sees it
  uint64_t begin;      // locus_read_begin[l]
  int32_t n_kept, n_alleles;
  int32_t size[2], lo[2], hi[2];
  int32_t flipped, pad;
};

__device__ inline double nan_none() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ inline int popc64(uint64_t v) { return __popcll((unsigned long long)v); }
__device__ inline double readlane_f64(double v, int lane) {  // lane is wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// ENC 0: one base per byte; 1: TRGT_READS_BAM4, two per byte, first base in the high nibble
template <int ENC>
__device__ inline uint32_t base_code(uint32_t w, int j) {
  if (ENC) { const uint32_t b = (w >> (8 * (j >> 1))) & 255u; return (j & 1) ? (b & 15u) : (b >> 4); }
  return (w >> (8 * j)) & 255u;
}

template <int ENC>
__global__ void __launch_bounds__(256) tr_meth_kernel(const uint8_t* __restrict__ reads, const uint8_t* __restrict__ calls, const Job* __restrict__ jobs, uint32_t n_jobs,
                                                      double* __restrict__ level, int32_t* __restrict__ span_len, double* __restrict__ read_meth, unsigned int* __restrict__ flag) {
  constexpr int BPL = ENC ? 8 : 4;   // bases in a lane's dword
  constexpr int STEP = 64 * BPL;     // bases of one wave-wide load
  constexpr uint32_t C = ENC ? 2u : (uint32_t)'C', G = ENC ? 4u : (uint32_t)'G';
  const uint32_t job = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (job >= n_jobs) return;
  const int lane = (int)(threadIdx.x & 63u);
  const Job jb = jobs[job];
  double result = nan_none();
  if (jb.n_meth != 0 && jb.s1 > jb.s0) {
    const uintptr_t p = (uintptr_t)(reads + jb.base_off), a0 = p & ~(uintptr_t)3;
    const uint32_t* __restrict__ wp = (const uint32_t*)a0;
    const int64_t lead = (int64_t)(p - a0) * (ENC ? 2 : 1);                  // bases of the first dword that lie in front of the read
    const int64_t lim = min((int64_t)jb.len - 1, (int64_t)jb.s1);            // a CpG counts at 0 <= pos < lim; base lim is the last one read
    const int64_t steps = (lim + lead) / STEP + 1;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    double total = 0.0;
    uint32_t in_span = 0, run = 0;   // CpGs inside the span so far; CpGs of the read in front of this step
    bool bad = false;
    int64_t pos0 = (int64_t)lane * BPL - lead;   // position of the lane's first base
    uint32_t cur = pos0 <= lim ? wp[lane] : 0u;
    for (int64_t t = 0; t < steps; ++t, pos0 += STEP) {
      const uint32_t nxt = (t + 1 < steps && pos0 + STEP <= lim) ? wp[(size_t)(t + 1) * 64 + lane] : 0u;
      // the base behind the lane's last one: the neighbour's first, or the next step's first
      const uint32_t beside = __shfl_down(cur, 1);
      const uint32_t ahead = base_code<ENC>(lane == 63 ? (uint32_t)__builtin_amdgcn_readlane((int)nxt, 0) : beside, 0);
      uint32_t m = 0;
#pragma unroll
      for (int j = 0; j < BPL; ++j) {
        const uint32_t c = base_code<ENC>(cur, j), g = j + 1 < BPL ? base_code<ENC>(cur, j + 1) : ahead;
        const int64_t pos = pos0 + j;
        if (c == C && g == G && pos >= 0 && pos < lim) m |= 1u << j;
      }
      const uint32_t n = (uint32_t)__popc(m);   // at most BPL / 2
      const uint64_t b0 = __ballot(n & 1u), b1 = __ballot(n & 2u), b2 = __ballot(n & 4u);
      const int64_t step_end = t * STEP - lead + STEP;   // first position behind this step (wave-uniform)
      if (step_end > (int64_t)jb.s0) {
        const int64_t shift = (int64_t)jb.s0 - pos0;
        const uint32_t s = shift <= 0 ? m : shift >= BPL ? 0u : (m & (~0u << shift));
        const uint32_t pre = run + (uint32_t)(popc64(b0 & below) + 2 * popc64(b1 & below) + 4 * popc64(b2 & below));
        uint32_t packed = 0; int k = 0;
#pragma unroll
        for (int j = 0; j < BPL; ++j)
          if ((s >> j) & 1u) {
            const uint32_t idx = pre + (uint32_t)__popc(m & ((1u << j) - 1u));
            if (idx >= jb.n_meth) bad = true;
            else packed |= (uint32_t)calls[jb.meth_off + idx] << (8 * k);
            ++k;
          }
        if (__ballot(bad)) break;
        uint64_t todo = __ballot(s != 0u);
        while (todo) {   // position order: lane by lane, and inside a lane call by call
          const int L = __ffsll((unsigned long long)todo) - 1;
          todo &= todo - 1;
          const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)packed, L);
          const int cnt = __popc((uint32_t)__builtin_amdgcn_readlane((int)s, L));
          for (int q = 0; q < cnt; ++q) total += (double)((pk >> (8 * q)) & 255u) / 255.0;
          in_span += (uint32_t)cnt;
        }
      }
      run += (uint32_t)(popc64(b0) + 2 * popc64(b1) + 4 * popc64(b2));
      cur = nxt;
    }
    if (__ballot(bad)) { if (lane == 0) atomicMin(flag, jb.read); }
    else if (in_span) result = total / (double)in_span;
  }
  if (lane == 0) {
    level[jb.slot] = result;
    span_len[jb.slot] = jb.s1 - jb.s0;
    if (read_meth) read_meth[jb.read] = result;
  }
}

__global__ void __launch_bounds__(256) fill_none_kernel(double* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = nan_none();
}

__global__ void __launch_bounds__(256) allele_meth_kernel(const Locus* __restrict__ loci, uint32_t n_loci, const double* __restrict__ level, const int32_t* __restrict__ span_len,
                                                          double* __restrict__ allele_meth, int32_t* __restrict__ meth_reads) {
  const uint32_t l = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (l >= n_loci) return;
  const int lane = (int)(threadIdx.x & 63u);
  const Locus g = loci[l];
  double sum[2] = {0.0, 0.0};
  int32_t cnt[2] = {0, 0};
  for (int32_t base = 0; base < g.n_kept; base += 64) {
    const int32_t rank = base + lane;
    const bool there = rank < g.n_kept;
    const double lv = there ? level[g.begin + (uint64_t)rank] : nan_none();
    const int64_t len = there ? (int64_t)span_len[g.begin + (uint64_t)rank] : 0;
    bool first = false, second = false;
    if (lv == lv && g.n_alleles >= 1) {   // assign_read
      if (g.n_alleles == 1) first = true;
      else {
        const bool spans_1 = g.lo[0] <= len && len <= g.hi[0], spans_2 = g.lo[1] <= len && len <= g.hi[1];
        const int64_t d1 = len > g.size[0] ? len - g.size[0] : g.size[0] - len, d2 = len > g.size[1] ? len - g.size[1] : g.size[1] - len;
        if (d1 < d2 && spans_1) first = true;
        else if (d2 < d1 && spans_2) second = true;
        else if (g.size[0] == g.size[1] && spans_1) first = second = true;
      }
    }
    uint64_t todo[2] = {__ballot(first), __ballot(second)};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      cnt[a] += popc64(todo[a]);
      while (todo[a]) {   // rank order
        const int L = __ffsll((unsigned long long)todo[a]) - 1;
        todo[a] &= todo[a] - 1;
        sum[a] += readlane_f64(lv, L);
      }
    }
  }
  if (lane < 2) {   // output slot `lane` holds allele `src` of the genotype's own order
    const int src = (g.flipped && g.n_alleles == 2) ? 1 - lane : lane;
    const bool has = lane < g.n_alleles && cnt[src] > 0;
    allele_meth[2 * (size_t)l + lane] = has ? sum[src] / (double)cnt[src] : nan_none();
    if (meth_reads) meth_reads[2 * (size_t)l + lane] = lane < g.n_alleles ? cnt[src] : 0;
  }
}

}  // namespace meth
}  // namespace trgt

using namespace trgt;

extern "C" int trgt_locus_meth_kernel_ms(const trgt_hip_ctx* c, double out[2]) {
  if (!c || !out) return TRGT_ERR_INVALID;
  out[0] = c->meth_ms[0]; out[1] = c->meth_ms[1];
  return TRGT_OK;
}

extern "C" int trgt_locus_meth_batch(trgt_hip_ctx* c, const trgt_locus_batch_in* in, const trgt_locus_batch_out* res, const uint8_t* calls, const uint64_t* meth_off,
                                     const uint8_t* has_meth, double* allele_meth, int32_t* meth_reads, double* read_meth) {
  if (!c) return TRGT_ERR_INVALID;
  if (!in || !res) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: null argument");
  const int64_t nl = in->n_loci;
  if (nl < 0) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: n_loci %lld", (long long)nl);
  if (!in->locus_read_begin || !in->read_blob || !in->read_off || !in->read_len || !res->span_start || !res->span_end || !res->read_rank || !res->n_alleles || !res->ci ||
      !res->allele_len || !calls || !meth_off || !has_meth || !allele_meth)
    return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: null field (in: locus_read_begin, read_blob, read_off, read_len; res: span_start, span_end, read_rank, n_alleles, ci, allele_len; meth, meth_off, has_meth, allele_meth)");
  if (in->read_encoding != TRGT_READS_ASCII && in->read_encoding != TRGT_READS_BAM4) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: read_encoding %d", in->read_encoding);
  if (nl == 0) return TRGT_OK;
  const bool bam4 = in->read_encoding == TRGT_READS_BAM4;
  try {
    // ---- everything the kernels index with is checked here, on the host arrays: no input reaches a launch that could read outside a buffer
    const uint64_t* lrb = in->locus_read_begin;
    for (int64_t l = 0; l < nl; ++l) if (lrb[l] > lrb[l + 1]) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: locus_read_begin decreases at locus %lld", (long long)l);
    const uint64_t nr = lrb[nl];
    if (lrb[0] != 0 || nr > 0x7FFFFFF0ull) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: locus_read_begin must start at 0 and stay below 2^31 reads");
    for (uint64_t r = 0; r < nr; ++r) {
      if (meth_off[r] > meth_off[r + 1]) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: meth_off decreases at read %llu", (unsigned long long)r);
      if (meth_off[r + 1] - meth_off[r] > 0xFFFFFFFFull) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: read %llu has more than 2^32 - 1 calls", (unsigned long long)r);
    }
    std::vector<meth::Job> jobs;
    std::vector<meth::Locus> loci((size_t)nl);
    std::vector<uint8_t> seen;
    uint64_t lo = ~0ull, hi = 0;   // bytes of read_blob the jobs read
    for (int64_t l = 0; l < nl; ++l) {
      const uint64_t r0 = lrb[l], n = lrb[l + 1] - lrb[l];
      seen.assign((size_t)n, 0);
      int32_t kept = 0;
      for (uint64_t r = r0; r < r0 + n; ++r) {
        const int32_t rank = res->read_rank[r];
        if (rank < 0) continue;
        if ((uint64_t)rank >= n || seen[(size_t)rank]) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: read %llu has rank %d, which is %s", (unsigned long long)r, rank, (uint64_t)rank >= n ? "beyond the reads of its locus" : "taken by another read of its locus");
        seen[(size_t)rank] = 1; ++kept;
        const int32_t s0 = res->span_start[r], s1 = res->span_end[r];
        if (s0 < 0 || s0 > s1 || (uint64_t)(int64_t)s1 > (uint64_t)in->read_len[r])
          return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: read %llu has span (%d, %d) outside its %u bases", (unsigned long long)r, s0, s1, in->read_len[r]);
        const uint64_t nm = has_meth[r] ? meth_off[r + 1] - meth_off[r] : 0;
        jobs.push_back(meth::Job{in->read_off[r], meth_off[r], (uint32_t)r, in->read_len[r], s0, s1, (uint32_t)nm, (uint32_t)(r0 + (uint64_t)rank)});
        if (nm != 0 && s1 > s0) {
          const uint64_t bases = std::min<uint64_t>(in->read_len[r], (uint64_t)s1 + 1);
          lo = std::min(lo, in->read_off[r]); hi = std::max(hi, in->read_off[r] + (bam4 ? (bases + 1) / 2 : bases));
        }
      }
      for (int32_t k = 0; k < kept; ++k) if (!seen[(size_t)k]) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: the ranks of locus %lld are not 0 .. %d", (long long)l, kept - 1);
      meth::Locus& g = loci[(size_t)l];
      const int n_al = res->n_alleles[l];
      if (n_al < 0 || n_al > 2) return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: locus %lld has n_alleles %d", (long long)l, n_al);
      const bool flipped = res->flipped && res->flipped[l] && n_al == 2;
      g.begin = r0; g.n_kept = kept; g.n_alleles = n_al; g.flipped = flipped ? 1 : 0; g.pad = 0;
      for (int a = 0; a < 2; ++a) {   // allele a of the genotype's own order sits in output slot o
        const int o = flipped ? 1 - a : a;
        const bool there = a < n_al;
        g.size[a] = there ? (res->gt_size ? res->gt_size[2 * l + o] : (int32_t)res->allele_len[2 * l + o]) : 0;
        g.lo[a] = there ? res->ci[4 * l + 2 * o] : 0; g.hi[a] = there ? res->ci[4 * l + 2 * o + 1] : 0;
      }
    }
    const size_t nj = jobs.size();
    if (nj > 0xFFFFFFF0ull / 4) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_locus_meth_batch: too many kept reads in one call");
    TRGT_HIP_TRY(c, hipSetDevice(c->device));
    // ---- inputs: the blobs in place when they are device memory, else the bytes the jobs read, uploaded for the call
    const uint8_t *d_reads = in->read_blob, *d_calls = calls;
    int rc;
    if (!is_device_ptr(in->read_blob) && hi > lo) {
      lo &= ~(uint64_t)255;
      void* d = nullptr;
      if ((rc = dev_get(c, S_METH_READS, (size_t)(hi - lo) + 64, &d))) return rc;
      TRGT_HIP_TRY(c, hipMemcpyAsync(d, in->read_blob + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->stream));
      d_reads = (const uint8_t*)d;
      for (auto& j : jobs) j.base_off = (j.n_meth != 0 && j.s1 > j.s0) ? j.base_off - lo : 0;   // (the other jobs read no base)
    }
    if (!is_device_ptr(calls) && meth_off[nr] > 0) {
      void* d = nullptr;
      if ((rc = dev_get(c, S_METH_CALLS, (size_t)meth_off[nr] + 64, &d))) return rc;
      TRGT_HIP_TRY(c, hipMemcpyAsync(d, calls, (size_t)meth_off[nr], hipMemcpyHostToDevice, c->stream));
      d_calls = (const uint8_t*)d;
    }
    void *d_jobs = nullptr, *d_loci = nullptr, *d_level = nullptr, *d_len = nullptr, *d_flag = nullptr;
    if ((rc = dev_get(c, S_METH_JOBS, nj * sizeof(meth::Job), &d_jobs)) || (rc = dev_get(c, S_METH_LOCI, (size_t)nl * sizeof(meth::Locus), &d_loci)) ||
        (rc = dev_get(c, S_METH_LEVEL, (size_t)nr * sizeof(double), &d_level)) || (rc = dev_get(c, S_METH_LEN, (size_t)nr * sizeof(int32_t), &d_len)) ||
        (rc = dev_get(c, S_METH_FLAG, 16, &d_flag)))
      return rc;
    if (nj) TRGT_HIP_TRY(c, hipMemcpyAsync(d_jobs, jobs.data(), nj * sizeof(meth::Job), hipMemcpyHostToDevice, c->stream));
    TRGT_HIP_TRY(c, hipMemcpyAsync(d_loci, loci.data(), (size_t)nl * sizeof(meth::Locus), hipMemcpyHostToDevice, c->stream));
    TRGT_HIP_TRY(c, hipMemsetAsync(d_flag, 0xFF, 16, c->stream));
    DevOut<double> o_am, o_rm; DevOut<int32_t> o_n;
    if ((rc = o_am.init(c, S_METH_OUT, allele_meth, 2 * (size_t)nl)) || (rc = o_n.init(c, S_METH_NREADS, meth_reads, 2 * (size_t)nl)) ||
        (rc = o_rm.init(c, S_METH_PERREAD, read_meth, (size_t)nr)))
      return rc;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (c->timing) for (auto& e : ev) TRGT_HIP_TRY(c, hipEventCreate(&e));
    // ---- tr_meth_kernel: one wave per kept read
    if (o_rm.dev && nr) { hipLaunchKernelGGL(meth::fill_none_kernel, dim3((unsigned)std::min<uint64_t>(1024, nr / 256 + 1)), dim3(256), 0, c->stream, o_rm.dev, (size_t)nr); TRGT_HIP_TRY(c, hipGetLastError()); }
    if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[0], c->stream));
    if (nj) {
      const dim3 grid((unsigned)((nj + 3) / 4)), block(256);
      if (bam4) hipLaunchKernelGGL(meth::tr_meth_kernel<1>, grid, block, 0, c->stream, d_reads, d_calls, (const meth::Job*)d_jobs, (uint32_t)nj, (double*)d_level, (int32_t*)d_len, o_rm.dev, (unsigned int*)d_flag);
      else hipLaunchKernelGGL(meth::tr_meth_kernel<0>, grid, block, 0, c->stream, d_reads, d_calls, (const meth::Job*)d_jobs, (uint32_t)nj, (double*)d_level, (int32_t*)d_len, o_rm.dev, (unsigned int*)d_flag);
      TRGT_HIP_TRY(c, hipGetLastError());
    }
    if (c->timing) { TRGT_HIP_TRY(c, hipEventRecord(ev[1], c->stream)); TRGT_HIP_TRY(c, hipEventRecord(ev[2], c->stream)); }
    // ---- allele_meth_kernel: one wave per locus
    hipLaunchKernelGGL(meth::allele_meth_kernel, dim3((unsigned)((nl + 3) / 4)), dim3(256), 0, c->stream, (const meth::Locus*)d_loci, (uint32_t)nl, (const double*)d_level,
                       (const int32_t*)d_len, o_am.dev, o_n.dev);
    TRGT_HIP_TRY(c, hipGetLastError());
    if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[3], c->stream));
    uint32_t flag = 0xFFFFFFFFu;
    if ((rc = d2h(c, &flag, d_flag, 4, c->stream)) || (rc = o_am.finish(c)) || (rc = o_n.finish(c)) || (rc = o_rm.finish(c))) return rc;
    TRGT_HIP_TRY(c, trgt::stream_wait(c, c->stream));
    if (c->timing) {
      float ms = 0;
      c->meth_ms[0] = hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess ? ms : 0.0;
      c->meth_ms[1] = hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess ? ms : 0.0;
      for (auto& e : ev) c->retired_events.push_back(e);
    }
    if (flag != 0xFFFFFFFFu)
      return fail(c, TRGT_ERR_INVALID, "trgt_locus_meth_batch: read %u has malformed methylation profile (a CpG inside its span (%d, %d) lies beyond its %llu calls)", flag,
                  res->span_start[flag], res->span_end[flag], (unsigned long long)(meth_off[flag + 1] - meth_off[flag]));
    return TRGT_OK;
  } catch (const std::bad_alloc&) { return fail(c, TRGT_ERR_NOMEM, "out of host memory"); }
}
