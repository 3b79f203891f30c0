// trgt_amd/csrc/merge_exact.hip -- trgt_merge_exact_batch: merge_exact of `trgt merge` (src/merge/strategy/exact.rs:6-88) for a batch of
// sites (include/trgt_hip_merge.h).
//
//   merge_hash_kernel   per input allele a 64-bit hash and the first 8 bytes as a big-endian key, left in HBM.  A wave takes 64 alleles:
//                       those of up to `lane_max` bytes one per lane, the longer ones one after the other with a dword per lane and step.
//                       The hash is a SUM of mixed (dword, position) terms, so both forms give the same value.
//   merge_site_kernel   one workgroup per site (a wave when the call's largest device site has at most 64 alleles).  Length and hash of
//                       every allele sit in LDS.  REF check across entries; ALT de-duplication on (length, hash), the bytes compared in
//                       HBM wherever both agree; the distinct ALTs compacted and ranked by counting over pairs on (length, prefix key),
//                       going to HBM only on key ties; the overwrite rule (a REF whose bytes some ALT has maps to that ALT); allele_map,
//                       then gt_out, by all threads.
//
// Sequences are read as aligned dwords, head and tail shifted and masked, and compared as big-endian numbers: by the first differing
// BYTE ("AAAB" < "BAAA"; a little-endian dword compare says otherwise).  The hash only ever spares a comparison: where it agrees the
// bytes decide (TRGT_MERGE_HASH_BITS=4 on a developer context shows it).  Sites beyond SITE_LIMIT alleles, and nothing else, are done
// by merge::site_host (merge_host.hpp) inside the same call.
#include "common.hpp"
#include "merge_host.hpp"

#include <climits>

using trgt::fail;

namespace merge {

constexpr uint32_t SITE_LIMIT = 4096;       // input alleles per site on the device: 20 bytes of LDS each (80 KB of the CU's 160 KB) + the REF bit mask
constexpr uint32_t WAVE_CMP_MIN = 256;      // REFs of this many bytes and more are compared by a wave (64 dwords per step), shorter ones by a lane each
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t HAS_POS = 0x40000000u;   // s_dup[i]: a distinct ALT whose output position is known (low bits)

typedef unsigned long long u64;

struct HashArgs {
  const uint8_t* blob; const uint64_t* off; const uint32_t* len; uint64_t* hash; uint64_t* key;
  uint32_t n, lane_max; uint64_t hash_mask;
};

struct SiteArgs {
  const uint8_t* blob; const uint64_t* off; const uint32_t* len; const uint64_t* hash; const uint64_t* key;
  const uint32_t* site_list; const uint64_t* seb; const uint64_t* eab; const uint64_t* egb; const int32_t* gt; const uint64_t* slot;
  int32_t* status; int32_t* n_out; int32_t* src; int32_t* map; int32_t* gt_out; u64* n_cmp;
  uint32_t cap;   // LDS arrays hold this many alleles (the call's largest device site, rounded up to 64)
};

// The up to four bytes at p as a little-endian dword; bytes at and beyond `rem` (>= 1) read as 0.  Two aligned loads at the most, and only
// of dwords that hold a byte of the sequence.
static __device__ __forceinline__ uint32_t fetch_le(const uint8_t* p, uint32_t rem) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t head = (uint32_t)(a & 3u), sh = head * 8u;
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  uint32_t v = q[0] >> sh;
  if (head && rem > 4u - head) v |= q[1] << (32u - sh);
  if (rem < 4u) v &= (1u << (8u * rem)) - 1u;
  return v;
}
static __device__ __forceinline__ uint32_t fetch_be(const uint8_t* p, uint32_t rem) { return __builtin_bswap32(fetch_le(p, rem)); }

static __device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}
static __device__ __forceinline__ uint64_t hash_term(uint32_t v, uint32_t j) { return mix64((((uint64_t)j << 32) | v) + 0x9E3779B97F4A7C15ull); }
static __device__ __forceinline__ uint64_t prefix_key(const uint8_t* p, uint32_t len) {
  const uint32_t hi = len ? fetch_be(p, len) : 0u, lo = len > 4 ? fetch_be(p + 4, len - 4) : 0u;
  return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(256) merge_hash_kernel(const HashArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool live = i < a.n;
  const uint32_t len = live ? a.len[i] : 0u;
  const uint8_t* p = a.blob + (live ? a.off[i] : 0ull);
  const bool lng = live && len > a.lane_max;
  if (live && !lng) {   // one allele per lane
    uint64_t h = 0;
    for (uint32_t pos = 0, j = 0; pos < len; pos += 4, ++j) h += hash_term(fetch_le(p + pos, len - pos), j);
    a.hash[i] = mix64(h ^ len) & a.hash_mask;
    a.key[i] = prefix_key(p, len);
  }
  u64 todo = __ballot(lng);
  while (todo) {        // one allele per wave
    const int l = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t wl = __shfl(len, l);
    const uint8_t* wp = (const uint8_t*)(uintptr_t)__shfl((u64)(uintptr_t)p, l);
    uint64_t h = 0;
    for (uint32_t pos = lane * 4u, j = lane; pos < wl; pos += 256u, j += 64u) h += hash_term(fetch_le(wp + pos, wl - pos), j);
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
    if ((int)lane == l) { a.hash[i] = mix64(h ^ wl) & a.hash_mask; a.key[i] = prefix_key(wp, wl); }
  }
}

// -1 / 0 / 1: the `len` bytes at pa against those at pb, by the first differing byte.  One lane.
static __device__ __forceinline__ int lane_cmp(const uint8_t* pa, const uint8_t* pb, uint32_t len) {
  for (uint32_t pos = 0; pos < len; pos += 4) {
    const uint32_t x = fetch_be(pa + pos, len - pos), y = fetch_be(pb + pos, len - pos);
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}
// The same by a whole wave, 64 dwords per step; the arguments are wave-uniform and every lane gets the answer.
static __device__ __forceinline__ int wave_cmp(const uint8_t* pa, const uint8_t* pb, uint32_t len, uint32_t lane) {
  for (uint32_t base = 0; base < len; base += 256u) {
    const uint32_t pos = base + lane * 4u;
    const uint32_t x = pos < len ? fetch_be(pa + pos, len - pos) : 0u, y = pos < len ? fetch_be(pb + pos, len - pos) : 0u;
    const u64 diff = __ballot(x != y);
    if (diff) {
      const int l = __ffsll((long long)diff) - 1;
      return (uint32_t)__shfl((int)x, l) < (uint32_t)__shfl((int)y, l) ? -1 : 1;
    }
  }
  return 0;
}

__global__ void __launch_bounds__(256) merge_site_kernel(const SiteArgs a) {
  extern __shared__ __align__(16) unsigned char merge_lds[];
  __shared__ uint32_t sh_first_ref, sh_bad_ref, sh_nu, sh_ref_pos, sh_bad_gt;
  __shared__ u64 sh_cmp;
  uint64_t* s_hash = (uint64_t*)merge_lds;          // [cap]; behind the de-duplication: the prefix keys of the distinct ALTs, by list slot
  uint32_t* s_len = (uint32_t*)(s_hash + a.cap);    // [cap]
  uint32_t* s_dup = s_len + a.cap;                  // [cap] lowest equal ALT, then HAS_POS | output position for the distinct ones
  uint32_t* s_list = s_dup + a.cap;                 // [cap] the distinct ALTs; behind the ranking: the merged index of every allele
  uint32_t* s_isref = s_list + a.cap;               // [cap / 32] bit i: allele i is the REF of its entry
  const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u, wave = tid >> 6, n_waves = T >> 6;
  const uint32_t s = a.site_list[blockIdx.x];
  const uint64_t e0 = a.seb[s], e1 = a.seb[s + 1], a0 = a.eab[e0];
  const uint32_t n = (uint32_t)(a.eab[e1] - a0);
  const uint64_t slot = a.slot[s];
  u64 my_cmp = 0;   // byte comparisons of this thread that went to HBM

  if (tid == 0) { sh_first_ref = NONE; sh_bad_ref = NONE; sh_nu = 0; sh_ref_pos = 0; sh_bad_gt = 0; sh_cmp = 0; }
  for (uint32_t i = tid; i < n; i += T) { s_len[i] = a.len[a0 + i]; s_hash[i] = a.hash[a0 + i]; }
  for (uint32_t w = tid; w < (n + 31u) / 32u; w += T) s_isref[w] = 0;
  __syncthreads();
  for (uint64_t e = e0 + tid; e < e1; e += T) {
    const uint64_t b = a.eab[e];
    if (a.eab[e + 1] > b) { const uint32_t i = (uint32_t)(b - a0); atomicOr(&s_isref[i >> 5], 1u << (i & 31u)); atomicMin(&sh_first_ref, i); }
  }
  __syncthreads();
  const uint32_t r0 = sh_first_ref;
  if (r0 == NONE) {   // exact.rs:32
    if (tid == 0) { a.status[s] = TRGT_MERGE_NO_REF; a.n_out[s] = 0; }
    return;
  }
  auto is_ref = [&](uint32_t i) { return (s_isref[i >> 5] >> (i & 31u)) & 1u; };
  auto bytes = [&](uint32_t i) { return a.blob + a.off[a0 + i]; };

  // ---- exact.rs:13-26: every later REF against the first
  const uint32_t len0 = s_len[r0];
  const uint64_t hash0 = s_hash[r0];
  const uint8_t* p0 = bytes(r0);
  if (len0 < WAVE_CMP_MIN) {
    for (uint64_t e = e0 + tid; e < e1; e += T) {
      const uint64_t b = a.eab[e];
      const uint32_t i = (uint32_t)(b - a0);
      if (a.eab[e + 1] == b || i == r0) continue;
      bool bad = s_len[i] != len0 || s_hash[i] != hash0;
      if (!bad && len0) { ++my_cmp; bad = lane_cmp(p0, bytes(i), len0) != 0; }
      if (bad) atomicMin(&sh_bad_ref, i);
    }
  } else {
    for (uint64_t e = e0 + wave; e < e1; e += n_waves) {   // (wave-uniform)
      const uint64_t b = a.eab[e];
      const uint32_t i = (uint32_t)(b - a0);
      if (a.eab[e + 1] == b || i == r0) continue;
      bool bad = s_len[i] != len0 || s_hash[i] != hash0;
      if (!bad) { if (lane == 0) ++my_cmp; bad = wave_cmp(p0, bytes(i), len0, lane) != 0; }
      if (bad && lane == 0) atomicMin(&sh_bad_ref, i);
    }
  }
  __syncthreads();
  if (sh_bad_ref != NONE) {
    if (my_cmp) atomicAdd(&sh_cmp, my_cmp);
    __syncthreads();
    if (tid == 0) {
      a.status[s] = TRGT_MERGE_REF_MISMATCH; a.n_out[s] = 0;
      a.src[slot] = (int32_t)(a0 + r0); a.src[slot + 1] = (int32_t)(a0 + sh_bad_ref);
      if (sh_cmp) atomicAdd(a.n_cmp, sh_cmp);
    }
    return;
  }

  // ---- :27-29, the HashSet: every ALT finds the lowest ALT with its bytes
  // A lane walks the ALTs in front of its own to the next one of its length and hash; short sequences it compares itself, long ones
  // (WAVE_CMP_MIN bytes and more) the wave compares together, one after the other.  The loop is the wave's: it ends when every lane has.
  for (uint32_t base = wave * 64u; base < n; base += T) {
    const uint32_t i = base + lane;
    const bool alt = i < n && !is_ref(i);
    const uint32_t li = alt ? s_len[i] : 0u;
    const uint64_t hi = alt ? s_hash[i] : 0ull;
    const uint8_t* pi = alt ? bytes(i) : nullptr;
    uint32_t j = 0, rep = i;
    bool done = !alt;
    while (__any(!done)) {
      const uint8_t* pj = nullptr;
      if (!done) {
        while (j < i && (s_len[j] != li || s_hash[j] != hi || is_ref(j))) ++j;
        if (j >= i) done = true;                          // none in front: distinct
        else if (li == 0) { rep = j; done = true; }
        else { pj = bytes(j); ++my_cmp; }
      }
      const bool need = !done, by_wave = need && li >= WAVE_CMP_MIN;
      int c = 0;
      if (need && !by_wave) c = lane_cmp(pj, pi, li);
      u64 todo = __ballot(by_wave);
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int r = wave_cmp((const uint8_t*)(uintptr_t)__shfl((u64)(uintptr_t)pj, l), (const uint8_t*)(uintptr_t)__shfl((u64)(uintptr_t)pi, l), __shfl(li, l), lane);
        if ((int)lane == l) c = r;
      }
      if (need) { if (c == 0) { rep = j; done = true; } else ++j; }
    }
    if (i < n) s_dup[i] = rep;
  }
  __syncthreads();
  // ---- the distinct ALTs, compacted (their order in the list does not matter: ranks are counted), with their prefix keys
  for (uint32_t i = tid; i < n; i += T)
    if (!is_ref(i) && s_dup[i] == i) {
      const uint32_t u = atomicAdd(&sh_nu, 1u);
      s_list[u] = i;
      s_hash[u] = a.key[a0 + i];   // (the hashes in LDS are done with; the hash of a distinct ALT is read from HBM below)
    }
  __syncthreads();
  const uint32_t nu = sh_nu;
  // ---- :34-39: the position of a distinct ALT is 1 + the number of distinct ALTs in front of it by (length, bytes)
  if (tid == 0) a.src[slot] = (int32_t)(a0 + r0);
  for (uint32_t u = tid; u < nu; u += T) {
    const uint32_t i = s_list[u], li = s_len[i];
    const uint64_t ki = s_hash[u];
    const uint8_t* pi = nullptr;
    uint32_t rank = 0;
    for (uint32_t v = 0; v < nu; ++v) {
      if (v == u) continue;
      const uint32_t j = s_list[v], lj = s_len[j];
      bool less = lj < li;
      if (lj == li) {
        const uint64_t kj = s_hash[v];
        less = kj < ki;
        if (kj == ki && li > 8u) {   // (up to 8 bytes the key is the sequence, and two distinct ALTs differ)
          if (!pi) pi = bytes(i);
          ++my_cmp;
          less = lane_cmp(bytes(j) + 8, pi + 8, li - 8u) < 0;
        }
      }
      rank += less ? 1u : 0u;
    }
    const uint32_t pos = 1u + rank;
    a.src[slot + pos] = (int32_t)(a0 + i);
    s_dup[i] = HAS_POS | pos;
    // :41-45, the later equal key: an ALT with the bytes of the REF takes the REF's alleles
    if (li == len0 && a.hash[a0 + i] == hash0) {
      bool eq = true;
      if (li) { ++my_cmp; eq = lane_cmp(p0, pi ? pi : bytes(i), li) == 0; }
      if (eq) sh_ref_pos = pos;
    }
  }
  __syncthreads();
  // ---- allele_map
  const uint32_t ref_pos = sh_ref_pos;
  for (uint32_t i = tid; i < n; i += T) {
    uint32_t m = ref_pos;
    if (!is_ref(i)) { const uint32_t d = s_dup[i]; m = ((d & HAS_POS) ? d : s_dup[d]) & (HAS_POS - 1u); }
    a.map[a0 + i] = (int32_t)m;
    s_list[i] = m;
  }
  __syncthreads();
  // ---- :47-86: the genotype values of the site, the entry of each by bisection
  const uint64_t g0 = a.egb[e0], g1 = a.egb[e1];
  for (uint64_t g = g0 + tid; g < g1; g += T) {
    const int32_t v = a.gt[g];
    int32_t o = v;
    if (v != TRGT_MERGE_GT_VECTOR_END && v >= 2) {
      uint64_t lo = e0, hi = e1;   // the last entry that begins at or before g
      while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (a.egb[mid] <= g) lo = mid; else hi = mid; }
      const uint64_t b = a.eab[lo], cnt = a.eab[lo + 1] - b, idx = (uint64_t)(v >> 1) - 1;
      if (idx >= cnt) sh_bad_gt = 1;
      else o = (int32_t)(((s_list[(uint32_t)(b - a0 + idx)] + 1u) << 1) | (uint32_t)(v & 1));
    }
    a.gt_out[g] = o;
  }
  if (my_cmp) atomicAdd(&sh_cmp, my_cmp);
  __syncthreads();
  if (tid == 0) {
    a.status[s] = sh_bad_gt ? TRGT_MERGE_GT_OUT_OF_RANGE : 0;
    a.n_out[s] = sh_bad_gt ? 0 : (int32_t)(1u + nu);
    if (sh_cmp) atomicAdd(a.n_cmp, sh_cmp);
  }
}

static size_t site_lds_bytes(uint32_t cap) { return (size_t)cap * 20u + (size_t)(cap / 32u) * 4u; }

// The host twin over a list of sites; every output array is a host array of the call's full shape
static void run_host_sites(const trgt_merge_in* in, const uint8_t* blob, const std::vector<int64_t>& sites, const uint64_t* slot_begin, int32_t* status, int32_t* n_out, int32_t* src,
                           int32_t* map, int32_t* gt_out) {
  for (int64_t s : sites) site_host(in, blob, s, &status[s], &n_out[s], src + slot_begin[s], map, gt_out);
}

}  // namespace merge

extern "C" int32_t trgt_merge_site_alleles_limit(void) { return (int32_t)merge::SITE_LIMIT; }

extern "C" int trgt_merge_stats(const trgt_hip_ctx* c, int64_t out[4]) {
  if (!c || !out) return TRGT_ERR_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = c->merge_stats[i];
  return TRGT_OK;
}

extern "C" int trgt_merge_kernel_ms(const trgt_hip_ctx* c, double out[2]) {
  if (!c || !out) return TRGT_ERR_INVALID;
  out[0] = c->merge_ms[0]; out[1] = c->merge_ms[1];
  return TRGT_OK;
}

extern "C" int trgt_merge_exact_host(const trgt_merge_in* in, trgt_merge_out* out) {
  try {
    merge::Shape shape;
    std::string err;
    if (const int rc = merge::validate("trgt_merge_exact_host", in, out, &shape, &err)) { trgt::ctx_free_error(err.c_str()); return rc; }
    for (int64_t s = 0; s < in->n_sites; ++s)
      merge::site_host(in, in->allele_blob, s, &out->site_status[s], &out->out_n_alleles[s], out->out_allele_src + out->out_allele_begin[s], out->allele_map, out->gt_out);
    return TRGT_OK;
  } catch (const std::bad_alloc&) { trgt::ctx_free_error("out of host memory"); return TRGT_ERR_NOMEM; }
}

extern "C" int trgt_merge_exact_batch(trgt_hip_ctx* c, const trgt_merge_in* in, trgt_merge_out* out) {
  using namespace trgt;
  if (!c) return TRGT_ERR_INVALID;
  try {
    merge::Shape shape;
    std::string err;
    if (const int rc = merge::validate("trgt_merge_exact_batch", in, out, &shape, &err)) return fail(c, rc, "%s", err.c_str());
    TRGT_HIP_TRY(c, hipSetDevice(c->device));
    const int64_t ns = in->n_sites;
    const uint64_t ne = shape.n_entries, na = shape.n_alleles, ng = shape.n_gt, nsrc = shape.n_src;
    for (int i = 0; i < 4; ++i) c->merge_stats[i] = 0;
    c->merge_ms[0] = c->merge_ms[1] = 0.0;
    if (ns == 0) return TRGT_OK;

    // the sites of the device, and those beyond its ceiling
    std::vector<uint32_t> dev_sites;
    std::vector<int64_t> host_sites;
    uint64_t largest = 0;
    for (int64_t s = 0; s < ns; ++s) {
      const uint64_t n = merge::site_alleles(in, s);
      if (n > merge::SITE_LIMIT) host_sites.push_back(s);
      else { dev_sites.push_back((uint32_t)s); largest = std::max(largest, n); }
    }
    const bool blob_dev = is_device_ptr(in->allele_blob);
    std::vector<int32_t> h_status((size_t)ns, 0);
    uint64_t n_cmp = 0;
    float ms_hash = 0, ms_site = 0;

    DevOut<int32_t> o_status, o_nout, o_src, o_map, o_gt;
    if (!dev_sites.empty()) {
      const size_t nd = dev_sites.size();
      const uint8_t* d_blob = nullptr;
      if (blob_dev) d_blob = in->allele_blob;
      else {
        void* d = nullptr;
        if (int rc = dev_get(c, S_MERGE_BLOB, (size_t)in->blob_len + 8, &d)) return rc;
        if (in->blob_len) TRGT_HIP_TRY(c, hipMemcpyAsync(d, in->allele_blob, (size_t)in->blob_len, hipMemcpyHostToDevice, c->stream));
        d_blob = (const uint8_t*)d;
      }
      const uint64_t *d_off = nullptr, *d_seb = nullptr, *d_eab = nullptr, *d_egb = nullptr, *d_slot = nullptr;
      const uint32_t *d_len = nullptr, *d_list = nullptr;
      const int32_t* d_gt = nullptr;
      int rc;
      if ((rc = dev_in(c, S_MERGE_OFF, in->allele_off, (size_t)na, &d_off))) return rc;
      if ((rc = dev_in(c, S_MERGE_LEN, in->allele_len, (size_t)na, &d_len))) return rc;
      if ((rc = dev_in(c, S_MERGE_SEB, in->site_entry_begin, (size_t)ns + 1, &d_seb))) return rc;
      if ((rc = dev_in(c, S_MERGE_EAB, in->entry_allele_begin, (size_t)ne + 1, &d_eab))) return rc;
      if ((rc = dev_in(c, S_MERGE_EGB, in->entry_gt_begin, (size_t)ne + 1, &d_egb))) return rc;
      if ((rc = dev_in(c, S_MERGE_SLOT, out->out_allele_begin, (size_t)ns + 1, &d_slot))) return rc;
      if ((rc = dev_in(c, S_MERGE_GT, in->gt, (size_t)ng, &d_gt))) return rc;
      if ((rc = dev_in(c, S_MERGE_LIST, dev_sites.data(), nd, &d_list))) return rc;
      void *d_hash = nullptr, *d_key = nullptr, *d_cnt = nullptr;
      if ((rc = dev_get(c, S_MERGE_HASH, (size_t)na * 8, &d_hash))) return rc;
      if ((rc = dev_get(c, S_MERGE_KEY, (size_t)na * 8, &d_key))) return rc;
      if ((rc = dev_get(c, S_MERGE_CNT, 8, &d_cnt))) return rc;
      TRGT_HIP_TRY(c, hipMemsetAsync(d_cnt, 0, 8, c->stream));
      if ((rc = o_status.init(c, S_MERGE_STATUS, out->site_status, (size_t)ns))) return rc;
      if ((rc = o_nout.init(c, S_MERGE_NOUT, out->out_n_alleles, (size_t)ns))) return rc;
      if ((rc = o_src.init(c, S_MERGE_SRC, out->out_allele_src, (size_t)nsrc))) return rc;
      if ((rc = o_map.init(c, S_MERGE_MAP, out->allele_map, (size_t)na))) return rc;
      if ((rc = o_gt.init(c, S_MERGE_GTOUT, out->gt_out, (size_t)ng))) return rc;

      hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
      if (c->timing) for (auto& e : ev) TRGT_HIP_TRY(c, hipEventCreate(&e));
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[0], c->stream));
      if (na) {
        merge::HashArgs ha;
        ha.blob = d_blob; ha.off = d_off; ha.len = d_len; ha.hash = (uint64_t*)d_hash; ha.key = (uint64_t*)d_key;
        ha.n = (uint32_t)na; ha.lane_max = (uint32_t)c->knobs.merge_lane_max;
        ha.hash_mask = c->knobs.merge_hash_bits >= 64 ? ~0ull : ((1ull << c->knobs.merge_hash_bits) - 1ull);
        hipLaunchKernelGGL(merge::merge_hash_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, c->stream, ha);
        TRGT_HIP_TRY(c, hipGetLastError());
      }
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[1], c->stream));
      merge::SiteArgs sa;
      sa.blob = d_blob; sa.off = d_off; sa.len = d_len; sa.hash = (const uint64_t*)d_hash; sa.key = (const uint64_t*)d_key;
      sa.site_list = d_list; sa.seb = d_seb; sa.eab = d_eab; sa.egb = d_egb; sa.gt = d_gt; sa.slot = d_slot;
      sa.status = o_status.dev; sa.n_out = o_nout.dev; sa.src = o_src.dev; sa.map = o_map.dev; sa.gt_out = o_gt.dev; sa.n_cmp = (merge::u64*)d_cnt;
      sa.cap = (uint32_t)std::max<uint64_t>(64, (largest + 63) / 64 * 64);
      const size_t lds = merge::site_lds_bytes(sa.cap);
      const unsigned threads = largest <= 64 ? 64u : 256u;   // a wave per site suffices for small sites: the form of the call's largest
      if (lds > 48 * 1024) TRGT_HIP_TRY(c, hipFuncSetAttribute((const void*)merge::merge_site_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(merge::merge_site_kernel, dim3((unsigned)nd), dim3(threads), lds, c->stream, sa);
      TRGT_HIP_TRY(c, hipGetLastError());
      if (c->timing) TRGT_HIP_TRY(c, hipEventRecord(ev[2], c->stream));
      if ((rc = o_status.finish(c)) || (rc = o_nout.finish(c)) || (rc = o_src.finish(c)) || (rc = o_map.finish(c)) || (rc = o_gt.finish(c))) return rc;
      if (!o_status.staged && (rc = d2h(c, h_status.data(), o_status.dev, (size_t)ns * 4, c->stream))) return rc;
      if ((rc = d2h(c, &n_cmp, d_cnt, 8, c->stream))) return rc;
      TRGT_HIP_TRY(c, stream_wait(c, c->stream));
      if (o_status.staged) std::memcpy(h_status.data(), out->site_status, (size_t)ns * 4);
      if (c->timing) {
        (void)hipEventElapsedTime(&ms_hash, ev[0], ev[1]);
        (void)hipEventElapsedTime(&ms_site, ev[1], ev[2]);
        for (auto& e : ev) c->retired_events.push_back(e);
      }
    }

    if (!host_sites.empty()) {
      // the bytes of these sites on the host: the caller's blob, or the span of the sites' alleles fetched from HBM
      const uint8_t* h_blob = in->allele_blob;
      std::vector<uint8_t> keep;
      if (blob_dev) {
        uint64_t lo = UINT64_MAX, hi = 0;
        for (int64_t s : host_sites)
          for (uint64_t a = in->entry_allele_begin[in->site_entry_begin[s]]; a < in->entry_allele_begin[in->site_entry_begin[s + 1]]; ++a) {
            lo = std::min(lo, in->allele_off[a]); hi = std::max(hi, in->allele_off[a] + in->allele_len[a]);
          }
        keep.resize((size_t)(hi - lo) + 1);
        if (hi > lo) TRGT_HIP_TRY(c, hipMemcpy(keep.data(), in->allele_blob + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost));
        h_blob = keep.data() - lo;
      }
      // results in host arrays of the call's shape; what the caller keeps in HBM is patched site by site
      struct Arr { int32_t* user; size_t n; bool dev; std::vector<int32_t> tmp; int32_t* p; };
      Arr st{out->site_status, (size_t)ns}, no{out->out_n_alleles, (size_t)ns}, sr{out->out_allele_src, (size_t)nsrc}, mp{out->allele_map, (size_t)na}, go{out->gt_out, (size_t)ng};
      for (Arr* x : {&st, &no, &sr, &mp, &go}) {
        x->dev = is_device_ptr(x->user);
        if (x->dev) { x->tmp.assign(x->n + 1, 0); x->p = x->tmp.data(); } else x->p = x->user;
      }
      merge::run_host_sites(in, h_blob, host_sites, out->out_allele_begin, st.p, no.p, sr.p, mp.p, go.p);
      for (int64_t s : host_sites) {
        h_status[(size_t)s] = st.p[s];
        const uint64_t e0 = in->site_entry_begin[s], e1 = in->site_entry_begin[s + 1];
        const uint64_t a0 = in->entry_allele_begin[e0], a1 = in->entry_allele_begin[e1], g0 = in->entry_gt_begin[e0], g1 = in->entry_gt_begin[e1];
        const uint64_t b0 = out->out_allele_begin[s], b1 = out->out_allele_begin[s + 1];
        if (st.dev) TRGT_HIP_TRY(c, hipMemcpy(st.user + s, st.p + s, 4, hipMemcpyHostToDevice));
        if (no.dev) TRGT_HIP_TRY(c, hipMemcpy(no.user + s, no.p + s, 4, hipMemcpyHostToDevice));
        if (sr.dev && b1 > b0) TRGT_HIP_TRY(c, hipMemcpy(sr.user + b0, sr.p + b0, (size_t)(b1 - b0) * 4, hipMemcpyHostToDevice));
        if (mp.dev && a1 > a0) TRGT_HIP_TRY(c, hipMemcpy(mp.user + a0, mp.p + a0, (size_t)(a1 - a0) * 4, hipMemcpyHostToDevice));
        if (go.dev && g1 > g0) TRGT_HIP_TRY(c, hipMemcpy(go.user + g0, go.p + g0, (size_t)(g1 - g0) * 4, hipMemcpyHostToDevice));
      }
    }

    c->merge_stats[0] = (int64_t)dev_sites.size();
    c->merge_stats[1] = (int64_t)host_sites.size();
    for (int64_t s = 0; s < ns; ++s) c->merge_stats[2] += h_status[(size_t)s] != 0;
    c->merge_stats[3] = (int64_t)n_cmp;
    c->merge_ms[0] = ms_hash; c->merge_ms[1] = ms_site;
    return TRGT_OK;
  } catch (const std::bad_alloc&) { return fail(c, TRGT_ERR_NOMEM, "out of host memory"); }
}
