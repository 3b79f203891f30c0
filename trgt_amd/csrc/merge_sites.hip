// trgt_amd/csrc/merge_sites.hip -- trgt_merge_sites_batch: merge_variants / merge_variant of `trgt merge` (src/merge/vcf_processor.rs)
// up to the call of merge_exact, for one contig (include/trgt_hip_merge_sites.h).
//
//   merge_sites_key_kernel     one thread per record: the rank k among the records of its file at its position (index minus the lower bound
//                              of pos inside the file, by bisection), the key pos << 24 | k.
//   merge_sites_hist_kernel,   a stable LSD radix sort of the (key, record) pairs, 8-bit digits, only the digits in which two keys of the
//   ..._offsets_kernel,        call can differ (the host has pos).  A wave owns a tile of 1 024 consecutive pairs: its 256 counts, one scan
//   ..._scatter_kernel         over (digit, tile), and a scatter that ranks the 64 pairs of a step among their equals by ballots.
//   merge_sites_flag_kernel,   key != predecessor -> flag -> scan -> site index; record_site, site_pos, site_template, entry_record, and the
//   ..._head_kernel            first sorted place of every site.  Records are numbered file after file and the sort is stable, so the sorted
//                              order IS the entry order of the present records, and a site's first record is its template.
//   merge_sites_fill_kernel    one workgroup per site.  Threads over the site's records: the padding test, the entries' allele and genotype
//                              begins (a scan of the allele counts in sorted order gives them).  Threads over the sample axis: the five rows
//                              and sample_src, dword stores coalesced over the samples; the stage status.
//   merge_sites_allele_kernel  one thread per output allele: its record by bisection in the scanned counts, allele_src, allele_len.
//   merge_sites_copy_kernel    only with a pre-1.0 file, behind a scan of the lengths: short alleles one per lane, long ones one per wave;
//                              aligned dword stores, byte stores at the two edges.
//
// The scans are common.hpp's block_prefix_u32 (one workgroup).  No float instruction touches a row value except legacy_am's division.
#include "common.hpp"
#include "merge_sites_host.hpp"

using trgt::fail;

namespace merge_sites {

typedef unsigned long long u64;
constexpr uint32_t TILE = 1024;          // pairs per wave in the sort
constexpr uint32_t COPY_LANE_MAX = 64;   // alleles of up to this many bytes are copied one per lane, longer ones one per wave

// pool slots (common.hpp: S_MSITES_0 .. S_MSITES_LAST)
enum {
  M_POS = trgt::S_MSITES_0, M_RECFILE, M_FRB, M_RAB, M_KEY_A, M_KEY_B, M_IDX_A, M_IDX_B, M_HIST, M_TILEOFF, M_FLAG, M_CNT, M_SITEOF, M_ABEGIN, M_FIRST, M_RECSITE,
  M_PREV1, M_AMINT, M_SAMPLEOFF, M_COLFILE, M_FILERS, M_PADBASE, M_INOFF, M_INLEN, M_INBLOB, M_W0, M_B0 = M_W0 + 5, M_V0 = M_B0 + 5, M_PADSORTED = M_V0 + 5, M_ALLELEREC, M_COUNTER,
  M_O_POS, M_O_TEMPLATE, M_O_STATUS, M_O_ENTRYREC, M_O_SEB, M_O_EAB, M_O_OFF, M_O_LEN, M_O_SRC, M_O_EGB, M_O_ROW0, M_O_SAMPLESRC = M_O_ROW0 + 5, M_O_BLOB, M_END
};
static_assert(M_END == trgt::S_MSITES_LAST + 1, "S_MSITES_LAST in common.hpp is the last slot of this list");

struct DevField { const uint8_t* width; const uint64_t* begin; const uint32_t* values; };

__global__ void __launch_bounds__(256) merge_sites_key_kernel(const int64_t* __restrict__ pos, const uint32_t* __restrict__ rec_file, const uint64_t* __restrict__ frb,
                                                              uint64_t* __restrict__ key, uint32_t* __restrict__ idx, uint32_t n) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const int64_t p = pos[r];
  uint32_t lo = (uint32_t)frb[rec_file[r]], hi = r;   // the first record of the file at p lies in [lo, hi]
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (pos[mid] < p) lo = mid + 1u; else hi = mid; }
  key[r] = ((uint64_t)p << RANK_BITS) | (uint64_t)(r - lo);
  idx[r] = r;
}

// ---- the sort.  hist[d * n_tiles + tile]: pairs of the tile with digit d
__global__ void __launch_bounds__(256) merge_sites_hist_kernel(const uint64_t* __restrict__ key, uint32_t* __restrict__ hist, uint32_t n, uint32_t n_tiles, uint32_t shift) {
  __shared__ uint32_t cnt[4][256];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, tile = blockIdx.x * 4u + wave;
  for (uint32_t d = lane; d < 256u; d += 64u) cnt[wave][d] = 0;
  __syncthreads();
  if (tile < n_tiles) {
    const uint32_t b = tile * TILE, e = min(b + TILE, n);
    for (uint32_t i = b + lane; i < e; i += 64u) atomicAdd(&cnt[wave][(uint32_t)(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (tile < n_tiles)
    for (uint32_t d = lane; d < 256u; d += 64u) hist[d * n_tiles + tile] = cnt[wave][d];
}

__global__ void __launch_bounds__(1024) merge_sites_offsets_kernel(const uint32_t* __restrict__ v, uint64_t* __restrict__ off, uint64_t n) { trgt::block_prefix_u32(v, off, n); }

__global__ void __launch_bounds__(256) merge_sites_scatter_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ idx, uint64_t* __restrict__ key_out, uint32_t* __restrict__ idx_out,
                                                                  const uint64_t* __restrict__ tile_off, uint32_t n, uint32_t n_tiles, uint32_t shift) {
  __shared__ uint32_t base_all[4][256];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, tile = blockIdx.x * 4u + wave;
  if (tile >= n_tiles) return;   // (no workgroup barrier below: a wave works on its own 256 counters)
  volatile uint32_t* base = base_all[wave];
  for (uint32_t d = lane; d < 256u; d += 64u) base[d] = (uint32_t)tile_off[d * n_tiles + tile];
  const u64 below = (1ull << lane) - 1ull;
  const uint32_t b = tile * TILE, e = min(b + TILE, n);
  for (uint32_t at = b; at < e; at += 64u) {   // (wave-uniform)
    const uint32_t i = at + lane;
    const bool live = i < e;
    const uint64_t k = live ? key[i] : 0ull;
    const uint32_t d = (uint32_t)(k >> shift) & 255u;
    u64 peers = __ballot(live);   // the live lanes with this lane's digit
#pragma unroll
    for (uint32_t bit = 0; bit < 8u; ++bit) {
      const u64 m = __ballot(live && ((d >> bit) & 1u));
      peers &= ((d >> bit) & 1u) ? m : ~m;
    }
    uint32_t to = 0;
    if (live) to = base[d] + (uint32_t)__popcll(peers & below);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // every read of the step is done before a counter moves ...
    __builtin_amdgcn_wave_barrier();
    if (live && (peers >> lane) <= 1ull) base[d] = base[d] + (uint32_t)__popcll(peers);   // the highest of the equals
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // ... and has moved before the next step reads it
    __builtin_amdgcn_wave_barrier();
    if (live) { key_out[to] = k; idx_out[to] = idx[i]; }
  }
}

// ---- the heads
__global__ void __launch_bounds__(256) merge_sites_flag_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ idx, const uint64_t* __restrict__ rab,
                                                               uint32_t* __restrict__ flag, uint32_t* __restrict__ cnt, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i == 0u || key[i] != key[i - 1u]) ? 1u : 0u;
  const uint32_t r = idx[i];
  cnt[i] = (uint32_t)(rab[r + 1u] - rab[r]);
}

struct HeadArgs {
  const uint64_t* key; const uint32_t* idx; const uint32_t* flag; const uint64_t* site_of;   // site_of: the exclusive scan of flag, [n + 1]
  const uint32_t* rec_file; int32_t* record_site; uint32_t* first;                           // first: [n + 1]
  int64_t* site_pos; int32_t* site_template; int32_t* entry_record;
  uint32_t n, n_files, cap;
};
__global__ void __launch_bounds__(256) merge_sites_head_kernel(const HeadArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t t = (uint32_t)a.site_of[i + 1u] - 1u, r = a.idx[i];
  a.record_site[r] = (int32_t)t;
  if (a.flag[i]) a.first[t] = i;
  if (i == a.n - 1u) a.first[t + 1u] = a.n;
  if (t < a.cap) {   // (the site arrays hold cap sites; a call whose sites do not fit delivers none of them)
    if (a.flag[i]) { a.site_pos[t] = (int64_t)(a.key[i] >> RANK_BITS); a.site_template[t] = (int32_t)r; }
    a.entry_record[t * a.n_files + a.rec_file[r]] = (int32_t)r;
  }
}

// ---- the fill
struct FillArgs {
  const uint32_t* idx; const uint32_t* first; const uint64_t* abegin; const uint32_t* rec_file; const uint64_t* frb;
  const uint8_t* pre_v1; const uint8_t* am_is_int; const uint32_t* sample_off; const uint32_t* col_file; const uint32_t* file_rs;
  const int32_t* entry_record;
  DevField fl[5];
  uint32_t* rows[5]; int32_t* sample_src; int32_t* status; uint64_t* seb; uint64_t* eab; uint64_t* egb; uint8_t* pad_sorted; u64* n_padded;
  uint32_t n_files, S, n_sites, n_records;
};

__global__ void __launch_bounds__(256) merge_sites_fill_kernel(const FillArgs a) {
  __shared__ uint32_t sh_ragged, sh_padded;
  const uint32_t tid = threadIdx.x, t = blockIdx.x, F = a.n_files, S = a.S;
  if (tid == 0) { sh_ragged = 0; sh_padded = 0; }
  __syncthreads();
  const uint32_t i0 = a.first[t], i1 = a.first[t + 1u];

  // the site's records in entry order: add_padding_base (:350-388), and the allele begin of every entry up to and including theirs
  for (uint32_t i = i0 + tid; i < i1; i += 256u) {
    const uint32_t r = a.idx[i], f = a.rec_file[r];
    uint32_t pad = 0;
    if (a.pre_v1[f]) {
      const uint32_t w = a.fl[1].width[r];
      const uint32_t* v = a.fl[1].values + a.fl[1].begin[r];
      uint32_t x, y;
      const uint32_t len = slice2(v[0], w == 2u ? v[1] : (uint32_t)VEND_I, (uint32_t)VEND_I, &x, &y);
      if (len) {
        int32_t m = (int32_t)x;
        if (len == 2u) m = min(m, (int32_t)y);
        pad = m != 0 ? 1u : 0u;
      }
    }
    a.pad_sorted[i] = (uint8_t)pad;
    if (pad) atomicAdd(&sh_padded, 1u);
    const uint32_t f_from = i == i0 ? 0u : a.rec_file[a.idx[i - 1u]] + 1u;
    const uint64_t at = a.abegin[i];
    for (uint32_t g = f_from; g <= f; ++g) a.eab[t * F + g] = at;
    if (i == i1 - 1u) {   // the absent files behind the last record, and the begin of the next site's first entry when this is the last site
      const uint64_t end = a.abegin[i1];
      for (uint32_t g = f + 1u; g < F; ++g) a.eab[t * F + g] = end;
      if (t == a.n_sites - 1u) a.eab[(t + 1u) * F] = end;
    }
  }
  for (uint32_t f = tid; f < F; f += 256u) a.egb[t * F + f] = ((uint64_t)t * S + a.sample_off[f]) * 2ull;
  if (tid == 0) {
    a.seb[t] = (uint64_t)t * F;
    if (t == a.n_sites - 1u) { a.seb[t + 1u] = (uint64_t)(t + 1u) * F; a.egb[(t + 1u) * F] = (uint64_t)(t + 1u) * S * 2ull; }
  }

  // the sample axis: process_record (:452-462, :570-656) and process_missing_record (:464-484)
  for (uint32_t j = tid; j < S; j += 256u) {
    const uint32_t f = a.col_file[j], s0 = a.sample_off[f], s = j - s0, ncol = a.sample_off[f + 1u] - s0;
    const int32_t r = a.entry_record[t * F + f];
    const uint32_t o = (t * S + j) * 2u;
    if (r < 0) {
      a.rows[0][o] = 0u; a.rows[0][o + 1u] = (uint32_t)VEND_I;
      a.rows[1][o] = (uint32_t)MISSING_I; a.rows[1][o + 1u] = (uint32_t)VEND_I;
      a.rows[2][o] = (uint32_t)MISSING_I; a.rows[2][o + 1u] = (uint32_t)VEND_I;
      a.rows[3][o] = MISSING_F; a.rows[3][o + 1u] = VEND_F;
      a.rows[4][o] = MISSING_F; a.rows[4][o + 1u] = VEND_F;
      a.sample_src[t * S + j] = -1;
      continue;
    }
    const bool legacy_file = a.am_is_int[f] != 0;
    bool ragged = false;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const bool legacy = k == 4 && legacy_file;
      const uint32_t end = (k < 3 || legacy) ? (uint32_t)VEND_I : VEND_F;
      const uint32_t w = a.fl[k].width[r];
      const uint32_t* v = a.fl[k].values + a.fl[k].begin[r] + (uint64_t)s * w;
      uint32_t x, y;
      const uint32_t len = slice2(v[0], w == 2u ? v[1] : end, end, &x, &y);
      ragged |= len == 0u;
      if (legacy) { x = len >= 1u ? legacy_am(x) : VEND_F; y = len == 2u ? legacy_am(y) : VEND_F; }
      a.rows[k][o] = x; a.rows[k][o + 1u] = y;
    }
    if (ragged) sh_ragged = 1u;
    a.sample_src[t * S + j] = (int32_t)(a.file_rs[f] + ((uint32_t)r - (uint32_t)a.frb[f]) * ncol + s);
  }
  __syncthreads();
  if (tid == 0) {
    a.status[t] = sh_ragged ? TRGT_MERGE_SITE_RAGGED : 0;
    if (sh_padded) atomicAdd(a.n_padded, (u64)sh_padded);
  }
}

// ---- the alleles
struct AlleleArgs {
  const uint64_t* abegin; const uint32_t* idx; const uint64_t* rab; const uint8_t* pad_sorted; const uint64_t* in_off; const uint32_t* in_len;
  int32_t* src; uint32_t* len; uint64_t* off; uint32_t* allele_rec;
  uint32_t n_alleles, n_records, keep_off;   // keep_off: no pre-1.0 file, the offsets are the input's
};
__global__ void __launch_bounds__(256) merge_sites_allele_kernel(const AlleleArgs a) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= a.n_alleles) return;
  uint32_t lo = 1u, hi = a.n_records;   // the least j with abegin[j] > x (abegin[n_records] = n_alleles > x)
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (a.abegin[mid] > (uint64_t)x) hi = mid; else lo = mid + 1u; }
  const uint32_t i = lo - 1u, r = a.idx[i];
  const uint32_t s = (uint32_t)(a.rab[r] + ((uint64_t)x - a.abegin[i]));
  a.src[x] = (int32_t)s;
  a.len[x] = a.in_len[s] + a.pad_sorted[i];
  a.allele_rec[x] = r;
  if (a.keep_off) a.off[x] = a.in_off[s];
}

// n bytes from src to dst by the lanes `lane` of `nl`: byte stores up to dst's dword boundary, aligned dword stores (each from the two
// aligned source dwords that hold its bytes), byte stores for the rest.  Only dwords that hold a byte of the sequence are read.
static __device__ __forceinline__ void copy_span(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane, uint32_t nl) {
  const uint32_t head = min(n, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
  for (uint32_t k = lane; k < head; k += nl) dst[k] = src[k];
  const uint32_t nd = (n - head) / 4u;
  uint32_t* d4 = (uint32_t*)(dst + head);
  const uintptr_t sa = (uintptr_t)(src + head);
  const uint32_t sh = (uint32_t)(sa & 3u) * 8u;
  const uint32_t* q = (const uint32_t*)(sa & ~(uintptr_t)3);
  for (uint32_t k = lane; k < nd; k += nl) {
    uint32_t v = q[k] >> sh;
    if (sh) v |= q[k + 1u] << (32u - sh);
    d4[k] = v;
  }
  for (uint32_t k = head + nd * 4u + lane; k < n; k += nl) dst[k] = src[k];
}

struct CopyArgs {
  const uint8_t* in_blob; const uint64_t* in_off; const uint32_t* in_len; const int32_t* src; const uint32_t* len; const uint64_t* off; const uint32_t* allele_rec;
  const uint8_t* pad_base; uint8_t* out_blob; uint32_t n_alleles;
};
__global__ void __launch_bounds__(256) merge_sites_copy_kernel(const CopyArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  const bool live = x < a.n_alleles;
  uint32_t n = 0;
  uint8_t* dst = nullptr;
  const uint8_t* sp = nullptr;
  if (live) {
    const uint32_t s = (uint32_t)a.src[x];
    n = a.in_len[s];
    dst = a.out_blob + a.off[x];
    sp = a.in_blob + a.in_off[s];
    if (a.len[x] != n) { dst[0] = a.pad_base[a.allele_rec[x]]; ++dst; }
  }
  const bool lng = live && n > COPY_LANE_MAX;
  if (live && !lng) copy_span(dst, sp, n, 0u, 1u);
  u64 todo = __ballot(lng);
  while (todo) {   // one allele per wave
    const int l = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    copy_span((uint8_t*)(uintptr_t)__shfl((u64)(uintptr_t)dst, l), (const uint8_t*)(uintptr_t)__shfl((u64)(uintptr_t)sp, l), __shfl(n, l), lane, 64u);
  }
}

}  // namespace merge_sites

extern "C" int trgt_merge_sites_stats(const trgt_hip_ctx* c, int64_t out[4]) {
  if (!c || !out) return TRGT_ERR_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = c->merge_sites_stats[i];
  return TRGT_OK;
}

extern "C" int trgt_merge_sites_kernel_ms(const trgt_hip_ctx* c, double out[3]) {
  if (!c || !out) return TRGT_ERR_INVALID;
  for (int i = 0; i < 3; ++i) out[i] = c->merge_sites_ms[i];
  return TRGT_OK;
}

extern "C" int trgt_merge_sites_host(const trgt_merge_sites_in* in, trgt_merge_sites_out* out) {
  try {
    merge_sites::Plan plan;
    std::string err;
    if (const int rc = merge_sites::validate("trgt_merge_sites_host", in, out, &plan, &err)) { trgt::ctx_free_error(err.c_str()); return rc; }
    int64_t stats[4];
    const int rc = merge_sites::run_host(in, out, plan, stats);
    if (rc) trgt::ctx_free_error(merge::fmt("trgt_merge_sites_host: %lld sites, cap_sites is %lld", (long long)out->n_sites, (long long)out->cap_sites).c_str());
    return rc;
  } catch (const std::bad_alloc&) { trgt::ctx_free_error("out of host memory"); return TRGT_ERR_NOMEM; }
}

extern "C" int trgt_merge_sites_batch(trgt_hip_ctx* c, const trgt_merge_sites_in* in, trgt_merge_sites_out* out) {
  using namespace trgt;
  using namespace merge_sites;
  if (!c) return TRGT_ERR_INVALID;
  try {
    Plan plan;
    std::string err;
    if (const int rc = validate("trgt_merge_sites_batch", in, out, &plan, &err)) return fail(c, rc, "%s", err.c_str());
    TRGT_HIP_TRY(c, hipSetDevice(c->device));
    for (int i = 0; i < 4; ++i) c->merge_sites_stats[i] = 0;
    for (int i = 0; i < 3; ++i) c->merge_sites_ms[i] = 0.0;
    const uint64_t nr = plan.n_records, na = plan.n_alleles, S = plan.S, nf = (uint64_t)in->n_files;
    const uint64_t cap = (uint64_t)out->cap_sites;
    if (nr == 0) {
      out->n_sites = 0;
      if (cap) { out->site_entry_begin[0] = 0; out->entry_allele_begin[0] = 0; out->entry_gt_begin[0] = 0; out->blob_written = 0; }
      return TRGT_OK;
    }
    hipStream_t st = c->stream;
    const uint32_t n = (uint32_t)nr, n_tiles = (n + TILE - 1u) / TILE;
    const unsigned rec_blocks = (n + 255u) / 256u, tile_blocks = (n_tiles + 3u) / 4u;
    int rc;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t ns64 = 0, written = 0, n_padded = 0;   // destinations of d2h(): declared in front of the guard, so no copy is pending into them when they die
    // Every exit: an error return first waits for the stream, which delivers or drops the downloads staged so far (their destinations are
    // these locals and the caller's arrays, all still alive), and the events of a timed call are parked whichever way the call ends.
    struct Guard {
      trgt_hip_ctx* c; hipStream_t st; hipEvent_t* ev; bool done;
      ~Guard() {
        if (!done) (void)trgt::stream_wait(c, st);
        for (int i = 0; i < 4; ++i) if (ev[i]) c->retired_events.push_back(ev[i]);
      }
    } guard{c, st, ev, false};
    if (c->timing) for (auto& e : ev) TRGT_HIP_TRY(c, hipEventCreate(&e));

    // ---- grouping
    const int64_t* d_pos = nullptr; const uint32_t* d_recfile = nullptr; const uint64_t *d_frb = nullptr, *d_rab = nullptr;
    if ((rc = dev_in(c, M_POS, in->pos, (size_t)nr, &d_pos))) return rc;
    if ((rc = dev_in(c, M_RECFILE, plan.rec_file.data(), (size_t)nr, &d_recfile))) return rc;
    if ((rc = dev_in(c, M_FRB, in->file_record_begin, (size_t)nf + 1, &d_frb))) return rc;
    if ((rc = dev_in(c, M_RAB, in->record_allele_begin, (size_t)nr + 1, &d_rab))) return rc;
    void *key_a = nullptr, *key_b = nullptr, *idx_a = nullptr, *idx_b = nullptr, *d_hist = nullptr, *d_tileoff = nullptr, *d_flag = nullptr, *d_cnt = nullptr, *d_siteof = nullptr,
         *d_abegin = nullptr, *d_first = nullptr, *d_recsite = nullptr;
    if ((rc = dev_get(c, M_KEY_A, (size_t)nr * 8, &key_a)) || (rc = dev_get(c, M_KEY_B, (size_t)nr * 8, &key_b)) || (rc = dev_get(c, M_IDX_A, (size_t)nr * 4, &idx_a)) ||
        (rc = dev_get(c, M_IDX_B, (size_t)nr * 4, &idx_b)) || (rc = dev_get(c, M_HIST, (size_t)n_tiles * 256 * 4, &d_hist)) || (rc = dev_get(c, M_TILEOFF, ((size_t)n_tiles * 256 + 1) * 8, &d_tileoff)) ||
        (rc = dev_get(c, M_FLAG, (size_t)nr * 4, &d_flag)) || (rc = dev_get(c, M_CNT, (size_t)nr * 4, &d_cnt)) || (rc = dev_get(c, M_SITEOF, ((size_t)nr + 1) * 8, &d_siteof)) ||
        (rc = dev_get(c, M_ABEGIN, ((size_t)nr + 1) * 8, &d_abegin)) || (rc = dev_get(c, M_FIRST, ((size_t)nr + 1) * 4, &d_first)) || (rc = dev_get(c, M_RECSITE, (size_t)nr * 4, &d_recsite)))
      return rc;
    // the site arrays of the heads: staged for up to min(cap, n) sites (there are at most n)
    const uint64_t capn = std::min<uint64_t>(cap, nr);
    void *d_sitepos = nullptr, *d_template = nullptr, *d_entryrec = nullptr;
    if ((rc = dev_get(c, M_O_POS, (size_t)capn * 8, &d_sitepos)) || (rc = dev_get(c, M_O_TEMPLATE, (size_t)capn * 4, &d_template)) || (rc = dev_get(c, M_O_ENTRYREC, (size_t)(capn * nf) * 4, &d_entryrec))) return rc;
    if (capn * nf) TRGT_HIP_TRY(c, hipMemsetAsync(d_entryrec, 0xFF, (size_t)(capn * nf) * 4, st));

    if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(merge_sites_key_kernel, dim3(rec_blocks), dim3(256), 0, st, d_pos, d_recfile, d_frb, (uint64_t*)key_a, (uint32_t*)idx_a, n);
    TRGT_HIP_TRY(c, hipGetLastError());
    uint64_t* kin = (uint64_t*)key_a; uint64_t* kout = (uint64_t*)key_b;
    uint32_t* iin = (uint32_t*)idx_a; uint32_t* iout = (uint32_t*)idx_b;
    for (uint32_t shift = 0; shift < 64; shift += 8) {
      if (((plan.vary >> shift) & 255ull) == 0) continue;   // every key of the call has the same digit here
      hipLaunchKernelGGL(merge_sites_hist_kernel, dim3(tile_blocks), dim3(256), 0, st, kin, (uint32_t*)d_hist, n, n_tiles, shift);
      hipLaunchKernelGGL(merge_sites_offsets_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)d_hist, (uint64_t*)d_tileoff, (uint64_t)n_tiles * 256);
      hipLaunchKernelGGL(merge_sites_scatter_kernel, dim3(tile_blocks), dim3(256), 0, st, kin, iin, kout, iout, (const uint64_t*)d_tileoff, n, n_tiles, shift);
      TRGT_HIP_TRY(c, hipGetLastError());
      std::swap(kin, kout); std::swap(iin, iout);
    }
    hipLaunchKernelGGL(merge_sites_flag_kernel, dim3(rec_blocks), dim3(256), 0, st, kin, iin, d_rab, (uint32_t*)d_flag, (uint32_t*)d_cnt, n);
    hipLaunchKernelGGL(merge_sites_offsets_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)d_flag, (uint64_t*)d_siteof, (uint64_t)n);
    hipLaunchKernelGGL(merge_sites_offsets_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)d_cnt, (uint64_t*)d_abegin, (uint64_t)n);
    HeadArgs ha;
    ha.key = kin; ha.idx = iin; ha.flag = (const uint32_t*)d_flag; ha.site_of = (const uint64_t*)d_siteof; ha.rec_file = d_recfile; ha.record_site = (int32_t*)d_recsite;
    ha.first = (uint32_t*)d_first; ha.site_pos = (int64_t*)d_sitepos; ha.site_template = (int32_t*)d_template; ha.entry_record = (int32_t*)d_entryrec;
    ha.n = n; ha.n_files = (uint32_t)nf; ha.cap = (uint32_t)capn;
    hipLaunchKernelGGL(merge_sites_head_kernel, dim3(rec_blocks), dim3(256), 0, st, ha);
    TRGT_HIP_TRY(c, hipGetLastError());
    if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[1], st));
    if ((rc = d2h(c, &ns64, (const uint64_t*)d_siteof + nr, 8, st)) || (rc = d2h(c, out->record_site, d_recsite, (size_t)nr * 4, st))) return rc;
    TRGT_HIP_TRY(c, stream_wait(c, st));
    out->n_sites = (int64_t)ns64;
    if (ns64 > cap) { guard.done = true; return fail(c, TRGT_ERR_NOMEM, "trgt_merge_sites_batch: %llu sites, cap_sites is %llu", (unsigned long long)ns64, (unsigned long long)cap); }
    const uint32_t ns = (uint32_t)ns64;

    // ---- fill
    const uint8_t *d_prev1 = nullptr, *d_amint = nullptr, *d_padbase = nullptr;
    const uint32_t *d_sampleoff = nullptr, *d_colfile = nullptr, *d_filers = nullptr, *d_inlen = nullptr;
    const uint64_t* d_inoff = nullptr;
    if ((rc = dev_in(c, M_PREV1, in->pre_v1, (size_t)nf, &d_prev1)) || (rc = dev_in(c, M_AMINT, in->am_is_int, (size_t)nf, &d_amint)) ||
        (rc = dev_in(c, M_SAMPLEOFF, plan.sample_off.data(), (size_t)nf + 1, &d_sampleoff)) || (rc = dev_in(c, M_COLFILE, plan.col_file.data(), (size_t)S, &d_colfile)) ||
        (rc = dev_in(c, M_FILERS, plan.file_rs_begin.data(), (size_t)nf, &d_filers)) || (rc = dev_in(c, M_INOFF, in->allele_off, (size_t)na, &d_inoff)) ||
        (rc = dev_in(c, M_INLEN, in->allele_len, (size_t)na, &d_inlen)))
      return rc;
    if (plan.any_pre_v1 && in->pad_base && (rc = dev_in(c, M_PADBASE, in->pad_base, (size_t)nr, &d_padbase))) return rc;
    FillArgs fa;
    for (int k = 0; k < 5; ++k) {
      const trgt_merge_field* fl = fields(in, k);
      const uint32_t* vals = nullptr;
      if ((rc = dev_in(c, M_W0 + k, fl->width, (size_t)nr, &fa.fl[k].width)) || (rc = dev_in(c, M_B0 + k, fl->begin, (size_t)nr + 1, &fa.fl[k].begin)) ||
          (rc = dev_in(c, M_V0 + k, (const uint32_t*)fl->values, (size_t)fl->begin[nr], &vals)))
        return rc;
      fa.fl[k].values = vals;
    }
    void *d_padsorted = nullptr, *d_allelerec = nullptr, *d_counter = nullptr, *d_status = nullptr, *d_seb = nullptr, *d_eab = nullptr, *d_egb = nullptr, *d_off = nullptr, *d_len = nullptr, *d_src = nullptr, *d_gt = nullptr;
    const uint64_t n_entries = (uint64_t)ns * nf;
    if ((rc = dev_get(c, M_PADSORTED, (size_t)nr, &d_padsorted)) || (rc = dev_get(c, M_ALLELEREC, (size_t)na * 4, &d_allelerec)) || (rc = dev_get(c, M_COUNTER, 8, &d_counter)) ||
        (rc = dev_get(c, M_O_STATUS, (size_t)ns * 4, &d_status)) || (rc = dev_get(c, M_O_SEB, ((size_t)ns + 1) * 8, &d_seb)) || (rc = dev_get(c, M_O_EAB, ((size_t)n_entries + 1) * 8, &d_eab)) ||
        (rc = dev_get(c, M_O_EGB, ((size_t)n_entries + 1) * 8, &d_egb)) || (rc = dev_get(c, M_O_OFF, ((size_t)na + 1) * 8, &d_off)) || (rc = dev_get(c, M_O_LEN, (size_t)na * 4, &d_len)) ||
        (rc = dev_get(c, M_O_SRC, (size_t)na * 4, &d_src)) || (rc = dev_get(c, M_O_ROW0, (size_t)ns * S * 2 * 4, &d_gt)))
      return rc;
    TRGT_HIP_TRY(c, hipMemsetAsync(d_counter, 0, 8, st));
    DevOut<uint32_t> o_row[4];
    uint32_t* user_rows[4] = {(uint32_t*)out->al, (uint32_t*)out->sd, out->ap, out->am};
    for (int k = 0; k < 4; ++k) if ((rc = o_row[k].init(c, M_O_ROW0 + 1 + k, user_rows[k], (size_t)ns * S * 2))) return rc;
    DevOut<int32_t> o_ssrc;
    if ((rc = o_ssrc.init(c, M_O_SAMPLESRC, out->sample_src, (size_t)ns * S))) return rc;

    fa.idx = iin; fa.first = (const uint32_t*)d_first; fa.abegin = (const uint64_t*)d_abegin; fa.rec_file = d_recfile; fa.frb = d_frb;
    fa.pre_v1 = d_prev1; fa.am_is_int = d_amint; fa.sample_off = d_sampleoff; fa.col_file = d_colfile; fa.file_rs = d_filers; fa.entry_record = (const int32_t*)d_entryrec;
    fa.rows[0] = (uint32_t*)d_gt; for (int k = 0; k < 4; ++k) fa.rows[1 + k] = o_row[k].dev;
    fa.sample_src = o_ssrc.dev; fa.status = (int32_t*)d_status; fa.seb = (uint64_t*)d_seb; fa.eab = (uint64_t*)d_eab; fa.egb = (uint64_t*)d_egb;
    fa.pad_sorted = (uint8_t*)d_padsorted; fa.n_padded = (u64*)d_counter;
    fa.n_files = (uint32_t)nf; fa.S = (uint32_t)S; fa.n_sites = ns; fa.n_records = n;
    hipLaunchKernelGGL(merge_sites_fill_kernel, dim3(ns), dim3(256), 0, st, fa);
    TRGT_HIP_TRY(c, hipGetLastError());
    AlleleArgs aa;
    aa.abegin = (const uint64_t*)d_abegin; aa.idx = iin; aa.rab = d_rab; aa.pad_sorted = (const uint8_t*)d_padsorted; aa.in_off = d_inoff; aa.in_len = d_inlen;
    aa.src = (int32_t*)d_src; aa.len = (uint32_t*)d_len; aa.off = (uint64_t*)d_off; aa.allele_rec = (uint32_t*)d_allelerec;
    aa.n_alleles = (uint32_t)na; aa.n_records = n; aa.keep_off = plan.any_pre_v1 ? 0u : 1u;
    if (na) {
      hipLaunchKernelGGL(merge_sites_allele_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, aa);
      if (plan.any_pre_v1) hipLaunchKernelGGL(merge_sites_offsets_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)d_len, (uint64_t*)d_off, (uint64_t)na);
      TRGT_HIP_TRY(c, hipGetLastError());
    }
    if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[2], st));

    // ---- blob copy
    uint8_t* d_outblob = nullptr;
    bool blob_staged = false;
    if (plan.any_pre_v1 && na) {
      const uint8_t* d_inblob = nullptr;
      if (is_device_ptr(in->allele_blob)) d_inblob = in->allele_blob;
      else {
        void* d = nullptr;
        if ((rc = dev_get(c, M_INBLOB, (size_t)in->blob_len + 8, &d))) return rc;
        if (in->blob_len) TRGT_HIP_TRY(c, hipMemcpyAsync(d, in->allele_blob, (size_t)in->blob_len, hipMemcpyHostToDevice, st));
        d_inblob = (const uint8_t*)d;
      }
      if (is_device_ptr(out->allele_blob)) d_outblob = out->allele_blob;
      else {
        void* d = nullptr;
        if ((rc = dev_get(c, M_O_BLOB, (size_t)plan.blob_need + 8, &d))) return rc;
        d_outblob = (uint8_t*)d; blob_staged = true;
      }
      CopyArgs ca;
      ca.in_blob = d_inblob; ca.in_off = d_inoff; ca.in_len = d_inlen; ca.src = (const int32_t*)d_src; ca.len = (const uint32_t*)d_len; ca.off = (const uint64_t*)d_off;
      ca.allele_rec = (const uint32_t*)d_allelerec; ca.pad_base = d_padbase; ca.out_blob = d_outblob; ca.n_alleles = (uint32_t)na;
      hipLaunchKernelGGL(merge_sites_copy_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, ca);
      TRGT_HIP_TRY(c, hipGetLastError());
    }
    if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[3], st));
    if (plan.any_pre_v1 && na && (rc = d2h(c, &written, (const uint64_t*)d_off + na, 8, st))) return rc;

    // ---- delivery
    if ((rc = d2h(c, &n_padded, d_counter, 8, st)) || (rc = d2h(c, out->site_pos, d_sitepos, (size_t)ns * 8, st)) || (rc = d2h(c, out->site_template, d_template, (size_t)ns * 4, st)) ||
        (rc = d2h(c, out->site_stage_status, d_status, (size_t)ns * 4, st)) || (rc = d2h(c, out->entry_record, d_entryrec, (size_t)n_entries * 4, st)) ||
        (rc = d2h(c, out->site_entry_begin, d_seb, ((size_t)ns + 1) * 8, st)) || (rc = d2h(c, out->entry_allele_begin, d_eab, ((size_t)n_entries + 1) * 8, st)) ||
        (rc = d2h(c, out->entry_gt_begin, d_egb, ((size_t)n_entries + 1) * 8, st)) || (rc = d2h(c, out->allele_off, d_off, (size_t)na * 8, st)) ||
        (rc = d2h(c, out->allele_len, d_len, (size_t)na * 4, st)) || (rc = d2h(c, out->allele_src, d_src, (size_t)na * 4, st)) || (rc = d2h(c, out->gt, d_gt, (size_t)ns * S * 2 * 4, st)))
      return rc;
    for (int k = 0; k < 4; ++k) if ((rc = o_row[k].finish(c))) return rc;
    if ((rc = o_ssrc.finish(c))) return rc;
    TRGT_HIP_TRY(c, stream_wait(c, st));
    guard.done = true;   // (nothing is pending any more)
    if (blob_staged && written) TRGT_HIP_TRY(c, hipMemcpy(out->allele_blob, d_outblob, (size_t)written, hipMemcpyDeviceToHost));
    out->blob_written = written;
    c->merge_sites_stats[0] = (int64_t)ns;
    for (uint32_t t = 0; t < ns; ++t) c->merge_sites_stats[1] += out->site_stage_status[t] != 0;
    c->merge_sites_stats[2] = (int64_t)n_padded; c->merge_sites_stats[3] = (int64_t)written;
    if (c->timing) {
      float ms[3] = {0, 0, 0};
      for (int i = 0; i < 3; ++i) { (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]); c->merge_sites_ms[i] = ms[i]; }
    }
    return TRGT_OK;
  } catch (const std::bad_alloc&) { return fail(c, TRGT_ERR_NOMEM, "out of host memory"); }
}
