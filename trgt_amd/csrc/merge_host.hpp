// trgt_amd/csrc/merge_host.hpp -- the host side of the merge path (include/trgt_hip_merge.h) in plain C++, no HIP: the checks of a call
// (merge::validate, shared by trgt_merge_exact_batch and trgt_merge_exact_host) and the host twin of the kernels (merge::site_host:
// merge_exact, src/merge/strategy/exact.rs:6-88, for one site, by a sort).  merge_exact.hip includes it; it also compiles on its own.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trgt_hip.h"

namespace merge {

struct Shape { uint64_t n_entries = 0, n_alleles = 0, n_gt = 0, n_src = 0; };

static inline std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// alleles and ALT alleles of site s, and what its slot must hold
static inline uint64_t site_alleles(const trgt_merge_in* in, int64_t s) {
  return in->entry_allele_begin[in->site_entry_begin[s + 1]] - in->entry_allele_begin[in->site_entry_begin[s]];
}
static inline uint64_t site_slot_need(const trgt_merge_in* in, int64_t s) {
  uint64_t alts = 0, non_empty = 0;
  for (uint64_t e = in->site_entry_begin[s]; e < in->site_entry_begin[s + 1]; ++e) {
    const uint64_t n = in->entry_allele_begin[e + 1] - in->entry_allele_begin[e];
    if (n) { alts += n - 1; ++non_empty; }
  }
  return non_empty == 0 ? 0 : std::max<uint64_t>(1 + alts, non_empty >= 2 ? 2 : 1);
}

// Every check of a call, in the order the header lists them; the message names the first offender.  0, or a TRGT_ERR_* code.
static inline int validate(const char* fn, const trgt_merge_in* in, const trgt_merge_out* out, Shape* shape, std::string* err) {
  if (!in || !out) { *err = fmt("%s: null argument", fn); return TRGT_ERR_INVALID; }
  const int64_t ns = in->n_sites;
  if (ns < 0) { *err = fmt("%s: n_sites %lld", fn, (long long)ns); return TRGT_ERR_INVALID; }
  if (!in->site_entry_begin || !in->entry_allele_begin || !in->entry_gt_begin || !out->out_allele_begin) {
    *err = fmt("%s: null field (in: site_entry_begin, entry_allele_begin, entry_gt_begin; out: out_allele_begin)", fn); return TRGT_ERR_INVALID;
  }
  if (in->site_entry_begin[0] != 0) { *err = fmt("%s: site_entry_begin must start at 0", fn); return TRGT_ERR_INVALID; }
  for (int64_t s = 0; s < ns; ++s)
    if (in->site_entry_begin[s] > in->site_entry_begin[s + 1]) { *err = fmt("%s: site_entry_begin decreases at site %lld", fn, (long long)s); return TRGT_ERR_INVALID; }
  const uint64_t ne = in->site_entry_begin[ns];
  if (in->entry_allele_begin[0] != 0 || in->entry_gt_begin[0] != 0) { *err = fmt("%s: %s must start at 0", fn, in->entry_allele_begin[0] ? "entry_allele_begin" : "entry_gt_begin"); return TRGT_ERR_INVALID; }
  for (uint64_t e = 0; e < ne; ++e)
    if (in->entry_allele_begin[e] > in->entry_allele_begin[e + 1]) { *err = fmt("%s: entry_allele_begin decreases at entry %llu", fn, (unsigned long long)e); return TRGT_ERR_INVALID; }
  for (uint64_t e = 0; e < ne; ++e)
    if (in->entry_gt_begin[e] > in->entry_gt_begin[e + 1]) { *err = fmt("%s: entry_gt_begin decreases at entry %llu", fn, (unsigned long long)e); return TRGT_ERR_INVALID; }
  if (out->out_allele_begin[0] != 0) { *err = fmt("%s: out_allele_begin must start at 0", fn); return TRGT_ERR_INVALID; }
  for (int64_t s = 0; s < ns; ++s)
    if (out->out_allele_begin[s] > out->out_allele_begin[s + 1]) { *err = fmt("%s: out_allele_begin decreases at site %lld", fn, (long long)s); return TRGT_ERR_INVALID; }
  const uint64_t na = in->entry_allele_begin[ne], ng = in->entry_gt_begin[ne], nsrc = out->out_allele_begin[ns];
  const uint64_t most = 0x7FFFFFF0ull;
  if (na >= most || ng >= most || nsrc >= most || (uint64_t)ns >= most || ne >= most) { *err = fmt("%s: too many sites, entries, alleles or genotype values in one call", fn); return TRGT_ERR_UNSUPPORTED; }
  if ((na && (!in->allele_off || !in->allele_len || !out->allele_map)) || (in->blob_len && !in->allele_blob) || (ng && (!in->gt || !out->gt_out)) ||
      (ns && (!out->site_status || !out->out_n_alleles)) || (nsrc && !out->out_allele_src)) {
    *err = fmt("%s: null field (in: allele_off, allele_len, allele_blob, gt; out: site_status, out_n_alleles, out_allele_src, allele_map, gt_out)", fn); return TRGT_ERR_INVALID;
  }
  for (uint64_t a = 0; a < na; ++a)
    if (in->allele_off[a] > in->blob_len || in->allele_len[a] > in->blob_len - in->allele_off[a]) {
      *err = fmt("%s: allele %llu (offset %llu, %u bytes) ends beyond the blob of %llu bytes", fn, (unsigned long long)a, (unsigned long long)in->allele_off[a], in->allele_len[a], (unsigned long long)in->blob_len);
      return TRGT_ERR_INVALID;
    }
  for (uint64_t g = 0; g < ng; ++g)
    if (in->gt[g] < 0 && in->gt[g] != TRGT_MERGE_GT_VECTOR_END) { *err = fmt("%s: gt[%llu] is %d (negative, and not vector end)", fn, (unsigned long long)g, in->gt[g]); return TRGT_ERR_INVALID; }
  for (int64_t s = 0; s < ns; ++s) {
    const uint64_t need = site_slot_need(in, s), have = out->out_allele_begin[s + 1] - out->out_allele_begin[s];
    if (have < need) { *err = fmt("%s: the slot of site %lld holds %llu alleles, the site needs %llu", fn, (long long)s, (unsigned long long)have, (unsigned long long)need); return TRGT_ERR_INVALID; }
  }
  shape->n_entries = ne; shape->n_alleles = na; shape->n_gt = ng; shape->n_src = nsrc;
  return TRGT_OK;
}

// merge_exact for site s.  blob is indexed by allele_off (the caller may pass a pointer shifted so that only the site's bytes are
// there); src points at the site's slot; map and gt_out are the whole arrays.
static inline void site_host(const trgt_merge_in* in, const uint8_t* blob, int64_t s, int32_t* status, int32_t* n_out, int32_t* src, int32_t* map, int32_t* gt_out) {
  const uint64_t e0 = in->site_entry_begin[s], e1 = in->site_entry_begin[s + 1];
  auto bytes = [&](uint64_t a) { return blob + in->allele_off[a]; };
  auto same = [&](uint64_t a, uint64_t b) { return in->allele_len[a] == in->allele_len[b] && (in->allele_len[a] == 0 || std::memcmp(bytes(a), bytes(b), in->allele_len[a]) == 0); };
  *n_out = 0;
  // exact.rs:13-31: the REF of the first non-empty entry, every later one held to it; the ALTs collected
  int64_t ref = -1;
  std::vector<uint64_t> alts;
  for (uint64_t e = e0; e < e1; ++e) {
    const uint64_t a0 = in->entry_allele_begin[e], a1 = in->entry_allele_begin[e + 1];
    if (a0 == a1) continue;
    if (ref < 0) ref = (int64_t)a0;
    else if (!same((uint64_t)ref, a0)) { *status = TRGT_MERGE_REF_MISMATCH; src[0] = (int32_t)ref; src[1] = (int32_t)a0; return; }
    for (uint64_t a = a0 + 1; a < a1; ++a) alts.push_back(a);
  }
  if (ref < 0) { *status = TRGT_MERGE_NO_REF; return; }
  // :34-39: by length, then bytes; equals next to each other, the lowest input index first
  std::sort(alts.begin(), alts.end(), [&](uint64_t a, uint64_t b) {
    if (in->allele_len[a] != in->allele_len[b]) return in->allele_len[a] < in->allele_len[b];
    const int c = in->allele_len[a] ? std::memcmp(bytes(a), bytes(b), in->allele_len[a]) : 0;
    return c != 0 ? c < 0 : a < b;
  });
  int32_t n = 1, ref_pos = 0;
  src[0] = (int32_t)ref;
  for (size_t k = 0; k < alts.size(); ++k) {
    if (k == 0 || !same(alts[k - 1], alts[k])) {
      src[n] = (int32_t)alts[k];
      if (same((uint64_t)ref, alts[k])) ref_pos = n;   // :41-45: the later equal key overwrites the REF's 0
      ++n;
    }
    map[alts[k]] = n - 1;
  }
  for (uint64_t e = e0; e < e1; ++e)
    if (in->entry_allele_begin[e] != in->entry_allele_begin[e + 1]) map[in->entry_allele_begin[e]] = ref_pos;
  // :47-86
  for (uint64_t e = e0; e < e1; ++e) {
    const uint64_t a0 = in->entry_allele_begin[e], cnt = in->entry_allele_begin[e + 1] - a0;
    for (uint64_t g = in->entry_gt_begin[e]; g < in->entry_gt_begin[e + 1]; ++g) {
      const int32_t v = in->gt[g];
      if (v == TRGT_MERGE_GT_VECTOR_END || v < 2) { gt_out[g] = v; continue; }
      const uint64_t idx = (uint64_t)(v >> 1) - 1;
      if (idx >= cnt) { *status = TRGT_MERGE_GT_OUT_OF_RANGE; return; }
      gt_out[g] = ((map[a0 + idx] + 1) << 1) | (v & 1);
    }
  }
  *status = 0; *n_out = n;
}

}  // namespace merge
