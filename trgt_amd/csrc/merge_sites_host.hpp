// trgt_amd/csrc/merge_sites_host.hpp -- the host side of trgt_merge_sites_batch (include/trgt_hip_merge_sites.h) in plain C++, no HIP:
// the checks of a call (merge_sites::validate, shared by trgt_merge_sites_batch and trgt_merge_sites_host; it also leaves the small
// per-file tables both need) and the host twin of the kernels (merge_sites::run_host: merge_variants / merge_variant of
// src/merge/vcf_processor.rs up to the call of merge_exact, by a sort on one thread).  merge_sites.hip includes it; it also compiles on
// its own (tests/tools/merge_sites_check.cpp).
#pragma once
#include <climits>

#include "merge_host.hpp"

#if defined(__HIPCC__)
#define MERGE_SITES_HD __host__ __device__ __forceinline__
#else
#define MERGE_SITES_HD inline
#endif

namespace merge_sites {

using merge::fmt;

constexpr int32_t MISSING_I = INT32_MIN, VEND_I = INT32_MIN + 1;          // vcf_processor.rs:24-27
constexpr uint32_t MISSING_F = 0x7F800001u, VEND_F = 0x7F800002u;
constexpr uint64_t MOST = 0x7FFFFFF0ull;                                   // 32-bit indices in the kernels
constexpr int64_t POS_LIMIT = (int64_t)1 << 40;
constexpr uint32_t RANK_BITS = 24, RANK_LIMIT = (1u << RANK_BITS) - 1u;   // records of one file at one position

// The slice of one sample, cut at the first vector end, in the two-value form of the rows: returns its length (0: ragged); [a] -> [a, end].
// Values are 32-bit patterns; `end` is the field's vector end.
MERGE_SITES_HD uint32_t slice2(uint32_t v0, uint32_t v1, uint32_t end, uint32_t* o0, uint32_t* o1) {
  if (v0 == end) { *o0 = end; *o1 = end; return 0u; }
  *o0 = v0; *o1 = v1;
  return v1 == end ? 1u : 2u;
}
// process_am_field, :641-647.  The one float operation of the path: IEEE division, correctly rounded (no fast-math in this library).
MERGE_SITES_HD uint32_t legacy_am(uint32_t bits) {
  const int32_t i = (int32_t)bits;
  if (i == MISSING_I) return MISSING_F;
  const float q = (float)i / 255.0f;
  uint32_t u;
  __builtin_memcpy(&u, &q, 4);
  return u;
}

// What validate leaves for the work: the sizes, the key bits that vary, and the per-file / per-column tables
struct Plan {
  uint64_t n_records = 0, n_alleles = 0, S = 0, n_rec_samples = 0, blob_need = 0;
  bool any_pre_v1 = false;
  uint64_t vary = 0;                        // bits of the key pos << 24 | k in which two keys of the call can differ
  std::vector<uint32_t> rec_file;           // [n_records] the file of a record
  std::vector<uint32_t> col_file;           // [S] the file of a sample column
  std::vector<uint32_t> sample_off;         // [n_files + 1] first column of a file
  std::vector<uint32_t> file_rs_begin;      // [n_files] record-sample index of the file's first record, first sample
};

static inline const trgt_merge_field* fields(const trgt_merge_sites_in* in, int k) {
  const trgt_merge_field* f[5] = {&in->gt, &in->al, &in->sd, &in->ap, &in->am};
  return f[k];
}
static const char* const FIELD_NAME[5] = {"gt", "al", "sd", "ap", "am"};

// Every check of a call, in the order the header lists them; the message names the first offender.  0, or an error code.
static inline int validate(const char* fn, const trgt_merge_sites_in* in, const trgt_merge_sites_out* out, Plan* p, std::string* err) {
#define MS_FAIL(code, ...) do { *err = fmt(__VA_ARGS__); return code; } while (0)
  typedef unsigned long long ull;
  if (!in || !out) MS_FAIL(TRGT_ERR_INVALID, "%s: null argument", fn);
  const int64_t nf = in->n_files, cap = out->cap_sites;
  if (nf < 0) MS_FAIL(TRGT_ERR_INVALID, "%s: n_files %lld", fn, (long long)nf);
  if (cap < 0) MS_FAIL(TRGT_ERR_INVALID, "%s: cap_sites %lld", fn, (long long)cap);
  if (!in->file_record_begin || !in->record_allele_begin) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (file_record_begin, record_allele_begin)", fn);
  if (nf && (!in->n_samples || !in->pre_v1 || !in->am_is_int)) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (n_samples, pre_v1, am_is_int)", fn);
  for (int64_t f = 0; f < nf; ++f)
    if (in->n_samples[f] < 1) MS_FAIL(TRGT_ERR_INVALID, "%s: n_samples[%lld] is %d", fn, (long long)f, in->n_samples[f]);
  if (in->file_record_begin[0] != 0) MS_FAIL(TRGT_ERR_INVALID, "%s: file_record_begin must start at 0", fn);
  for (int64_t f = 0; f < nf; ++f)
    if (in->file_record_begin[f] > in->file_record_begin[f + 1]) MS_FAIL(TRGT_ERR_INVALID, "%s: file_record_begin decreases at file %lld", fn, (long long)f);
  const uint64_t nr = in->file_record_begin[nf];
  if (nr >= MOST || (uint64_t)nf >= MOST) MS_FAIL(TRGT_ERR_UNSUPPORTED, "%s: too many files or records in one call", fn);
  if (nr && (!in->pos || !out->record_site)) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (in: pos; out: record_site)", fn);
  if (in->record_allele_begin[0] != 0) MS_FAIL(TRGT_ERR_INVALID, "%s: record_allele_begin must start at 0", fn);
  for (uint64_t r = 0; r < nr; ++r)
    if (in->record_allele_begin[r] > in->record_allele_begin[r + 1]) MS_FAIL(TRGT_ERR_INVALID, "%s: record_allele_begin decreases at record %llu", fn, (ull)r);
  const uint64_t na = in->record_allele_begin[nr];
  if (na >= MOST) MS_FAIL(TRGT_ERR_UNSUPPORTED, "%s: too many alleles in one call", fn);
  if ((na && (!in->allele_off || !in->allele_len)) || (in->blob_len && !in->allele_blob)) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (allele_off, allele_len, allele_blob)", fn);

  // the tables
  p->sample_off.assign((size_t)nf + 1, 0);
  p->file_rs_begin.assign((size_t)nf, 0);
  uint64_t S = 0, nrs = 0;
  for (int64_t f = 0; f < nf; ++f) {
    if (S >= MOST || nrs >= MOST) break;
    p->sample_off[(size_t)f] = (uint32_t)S; p->file_rs_begin[(size_t)f] = (uint32_t)nrs;
    S += (uint64_t)in->n_samples[f];
    nrs += (in->file_record_begin[f + 1] - in->file_record_begin[f]) * (uint64_t)in->n_samples[f];
  }
  if (S >= MOST || nrs >= MOST) MS_FAIL(TRGT_ERR_UNSUPPORTED, "%s: too many samples or record-samples in one call", fn);
  p->sample_off[(size_t)nf] = (uint32_t)S;
  if (cap && ((uint64_t)cap >= MOST || (uint64_t)cap * std::max<uint64_t>((uint64_t)nf, 2 * S) >= MOST))
    MS_FAIL(TRGT_ERR_UNSUPPORTED, "%s: cap_sites %lld times the files or sample values of a site is beyond 32-bit indices", fn, (long long)cap);
  p->rec_file.resize((size_t)nr);
  p->col_file.resize((size_t)S);
  for (int64_t f = 0; f < nf; ++f) {
    for (uint64_t r = in->file_record_begin[f]; r < in->file_record_begin[f + 1]; ++r) p->rec_file[(size_t)r] = (uint32_t)f;
    for (uint32_t c = p->sample_off[(size_t)f]; c < p->sample_off[(size_t)f + 1]; ++c) p->col_file[c] = (uint32_t)f;
    if (in->pre_v1[f]) p->any_pre_v1 = true;
  }

  // the five fields
  for (int k = 0; k < 5; ++k) {
    const trgt_merge_field* fl = fields(in, k);
    if (!fl->begin || (nr && !fl->width)) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (%s.width, %s.begin)", fn, FIELD_NAME[k], FIELD_NAME[k]);
    if (fl->begin[0] != 0) MS_FAIL(TRGT_ERR_INVALID, "%s: %s.begin must start at 0", fn, FIELD_NAME[k]);
    for (uint64_t r = 0; r < nr; ++r) {
      const uint32_t w = fl->width[r];
      if (w == 0) MS_FAIL(TRGT_ERR_INVALID, "%s: %s.width[%llu] is 0", fn, FIELD_NAME[k], (ull)r);
      if (w > 2) MS_FAIL(TRGT_ERR_UNSUPPORTED, "%s: %s.width[%llu] is %u (at most 2 values per sample)", fn, FIELD_NAME[k], (ull)r, w);
      if (fl->begin[r + 1] < fl->begin[r]) MS_FAIL(TRGT_ERR_INVALID, "%s: %s.begin decreases at record %llu", fn, FIELD_NAME[k], (ull)r);
      const uint64_t want = (uint64_t)in->n_samples[p->rec_file[(size_t)r]] * w;
      if (fl->begin[r + 1] - fl->begin[r] != want)
        MS_FAIL(TRGT_ERR_INVALID, "%s: %s.begin gives record %llu %llu values, n_samples * width is %llu", fn, FIELD_NAME[k], (ull)r, (ull)(fl->begin[r + 1] - fl->begin[r]), (ull)want);
    }
    if (fl->begin[nr] && !fl->values) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (%s.values)", fn, FIELD_NAME[k]);
  }

  // positions, and the key bits that vary
  uint64_t or_pos = 0, and_pos = ~0ull, max_rank = 0;
  for (int64_t f = 0; f < nf; ++f) {
    uint64_t run = 0;
    for (uint64_t r = in->file_record_begin[f]; r < in->file_record_begin[f + 1]; ++r) {
      const int64_t q = in->pos[r];
      if (q < 0 || q >= POS_LIMIT) MS_FAIL(TRGT_ERR_INVALID, "%s: pos[%llu] is %lld, outside [0, 2^40)", fn, (ull)r, (long long)q);
      if (r > in->file_record_begin[f] && q < in->pos[r - 1]) MS_FAIL(TRGT_ERR_INVALID, "%s: pos[%llu] is %lld behind %lld: the position decreases inside file %lld", fn, (ull)r, (long long)q, (long long)in->pos[r - 1], (long long)f);
      run = (r > in->file_record_begin[f] && q == in->pos[r - 1]) ? run + 1 : 0;
      if (run >= RANK_LIMIT) MS_FAIL(TRGT_ERR_UNSUPPORTED, "%s: file %lld has more than 2^24 - 1 records at position %lld", fn, (long long)f, (long long)q);
      max_rank = std::max(max_rank, run);
      or_pos |= (uint64_t)q; and_pos &= (uint64_t)q;
    }
  }
  uint64_t rank_bits = 0;
  while (max_rank >> rank_bits) ++rank_bits;
  p->vary = nr ? (((or_pos ^ and_pos) << RANK_BITS) | ((1ull << rank_bits) - 1ull)) : 0;

  uint64_t sum_len = 0;
  for (uint64_t a = 0; a < na; ++a) {
    if (in->allele_off[a] > in->blob_len || in->allele_len[a] > in->blob_len - in->allele_off[a])
      MS_FAIL(TRGT_ERR_INVALID, "%s: allele %llu (offset %llu, %u bytes) ends beyond the blob of %llu bytes", fn, (ull)a, (ull)in->allele_off[a], in->allele_len[a], (ull)in->blob_len);
    sum_len += in->allele_len[a];
  }
  uint64_t pre_alleles = 0, pre_records = 0;
  for (int64_t f = 0; f < nf; ++f)
    if (in->pre_v1[f]) {
      pre_alleles += in->record_allele_begin[in->file_record_begin[f + 1]] - in->record_allele_begin[in->file_record_begin[f]];
      pre_records += in->file_record_begin[f + 1] - in->file_record_begin[f];
    }
  if (pre_records && !in->pad_base) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (pad_base)", fn);
  p->blob_need = p->any_pre_v1 ? sum_len + pre_alleles : 0;

  if (cap) {
    if (!out->site_pos || !out->site_template || !out->site_stage_status || !out->site_entry_begin || !out->entry_allele_begin || !out->entry_gt_begin || (nf && !out->entry_record))
      MS_FAIL(TRGT_ERR_INVALID, "%s: null field (out: site_pos, site_template, site_stage_status, entry_record, site_entry_begin, entry_allele_begin, entry_gt_begin)", fn);
    if (S && (!out->gt || !out->al || !out->sd || !out->ap || !out->am || !out->sample_src)) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (out: gt, al, sd, ap, am, sample_src)", fn);
    if (na && (!out->allele_off || !out->allele_len || !out->allele_src)) MS_FAIL(TRGT_ERR_INVALID, "%s: null field (out: allele_off, allele_len, allele_src)", fn);
    if (p->blob_need && (!out->allele_blob || out->blob_cap < p->blob_need))
      MS_FAIL(TRGT_ERR_INVALID, "%s: blob_cap is %llu, a call with a pre-1.0 file needs %llu bytes for these alleles", fn, (ull)(out->allele_blob ? out->blob_cap : 0), (ull)p->blob_need);
  }
  p->n_records = nr; p->n_alleles = na; p->S = S; p->n_rec_samples = nrs;
  return TRGT_OK;
#undef MS_FAIL
}

// The host twin.  stats: sites, sites with a status, padded records, blob bytes written.  TRGT_OK, or TRGT_ERR_NOMEM behind n_sites and
// record_site when the sites do not fit.
static inline int run_host(const trgt_merge_sites_in* in, trgt_merge_sites_out* out, const Plan& p, int64_t stats[4]) {
  const uint64_t nr = p.n_records, nf = (uint64_t)in->n_files, S = p.S;
  // ---- the sites: distinct keys in increasing order (the heap, :242-285)
  std::vector<std::pair<uint64_t, uint32_t>> order((size_t)nr);
  for (uint64_t f = 0; f < nf; ++f) {
    uint64_t rank = 0;
    for (uint64_t r = in->file_record_begin[f]; r < in->file_record_begin[f + 1]; ++r) {
      rank = (r > in->file_record_begin[f] && in->pos[r] == in->pos[r - 1]) ? rank + 1 : 0;
      order[(size_t)r] = {((uint64_t)in->pos[r] << RANK_BITS) | rank, (uint32_t)r};
    }
  }
  std::sort(order.begin(), order.end());
  std::vector<uint64_t> first;   // the first place in `order` of every site, and the end
  for (uint64_t i = 0; i < nr; ++i) {
    if (i == 0 || order[(size_t)i].first != order[(size_t)i - 1].first) first.push_back(i);
    out->record_site[order[(size_t)i].second] = (int32_t)(first.size() - 1);
  }
  const uint64_t ns = first.size();
  first.push_back(nr);
  out->n_sites = (int64_t)ns;
  for (int i = 0; i < 4; ++i) stats[i] = 0;
  if ((int64_t)ns > out->cap_sites) return TRGT_ERR_NOMEM;
  out->blob_written = 0;
  if (out->cap_sites == 0) return TRGT_OK;

  const trgt_merge_field* fl[5] = {&in->gt, &in->al, &in->sd, &in->ap, &in->am};
  uint32_t* rows[5] = {(uint32_t*)out->gt, (uint32_t*)out->al, (uint32_t*)out->sd, out->ap, out->am};
  uint64_t n_out_alleles = 0, blob_at = 0;
  out->site_entry_begin[0] = 0; out->entry_allele_begin[0] = 0; out->entry_gt_begin[0] = 0;
  for (uint64_t t = 0; t < ns; ++t) {
    out->site_pos[t] = (int64_t)(order[(size_t)first[t]].first >> RANK_BITS);
    out->site_template[t] = (int32_t)order[(size_t)first[t]].second;   // (records are numbered file after file: the first is the lowest file's)
    for (uint64_t f = 0; f < nf; ++f) out->entry_record[t * nf + f] = -1;
    for (uint64_t i = first[t]; i < first[t + 1]; ++i) out->entry_record[t * nf + p.rec_file[order[(size_t)i].second]] = (int32_t)order[(size_t)i].second;
    bool ragged = false;
    for (uint64_t f = 0; f < nf; ++f) {
      const uint64_t e = t * nf + f, ncol = (uint64_t)in->n_samples[f], col0 = t * S + p.sample_off[(size_t)f];
      const int32_t r = out->entry_record[e];
      if (r < 0) {   // process_missing_record, :464-484
        for (uint64_t i = 0; i < ncol; ++i) {
          const uint64_t o = (col0 + i) * 2;
          rows[0][o] = 0; rows[0][o + 1] = (uint32_t)VEND_I;
          rows[1][o] = rows[2][o] = (uint32_t)MISSING_I; rows[1][o + 1] = rows[2][o + 1] = (uint32_t)VEND_I;
          rows[3][o] = rows[4][o] = MISSING_F; rows[3][o + 1] = rows[4][o + 1] = VEND_F;
          out->sample_src[col0 + i] = -1;
        }
      } else {       // process_record, :452-462, :570-656
        uint32_t first_al_len = 0, first_al[2] = {0, 0};
        for (int k = 0; k < 5; ++k) {
          const uint32_t w = fl[k]->width[r];
          const uint32_t* v = (const uint32_t*)fl[k]->values + fl[k]->begin[r];
          const bool legacy = k == 4 && in->am_is_int[f];
          const uint32_t end = (k < 3 || legacy) ? (uint32_t)VEND_I : VEND_F;
          for (uint64_t i = 0; i < ncol; ++i) {
            uint32_t a, b;
            const uint32_t len = slice2(v[i * w], w == 2 ? v[i * w + 1] : end, end, &a, &b);
            if (len == 0) ragged = true;
            if (k == 1 && i == 0) { first_al_len = len; first_al[0] = a; first_al[1] = b; }
            if (legacy) { a = len >= 1 ? legacy_am(a) : VEND_F; b = len == 2 ? legacy_am(b) : VEND_F; }
            const uint64_t o = (col0 + i) * 2;
            rows[k][o] = a; rows[k][o + 1] = b;
          }
        }
        for (uint64_t i = 0; i < ncol; ++i) out->sample_src[col0 + i] = (int32_t)(p.file_rs_begin[(size_t)f] + ((uint64_t)r - in->file_record_begin[f]) * ncol + i);
        // add_padding_base, :350-388
        bool pad = false;
        if (in->pre_v1[f] && first_al_len) {
          int32_t m = (int32_t)first_al[0];
          if (first_al_len == 2) m = std::min(m, (int32_t)first_al[1]);
          pad = m != 0;
        }
        stats[2] += pad;
        for (uint64_t a = in->record_allele_begin[r]; a < in->record_allele_begin[r + 1]; ++a) {
          out->allele_src[n_out_alleles] = (int32_t)a;
          out->allele_len[n_out_alleles] = in->allele_len[a] + (pad ? 1u : 0u);
          if (p.any_pre_v1) {
            out->allele_off[n_out_alleles] = blob_at;
            if (pad) out->allele_blob[blob_at++] = in->pad_base[r];
            if (in->allele_len[a]) std::memcpy(out->allele_blob + blob_at, in->allele_blob + in->allele_off[a], in->allele_len[a]);
            blob_at += in->allele_len[a];
          } else out->allele_off[n_out_alleles] = in->allele_off[a];
          ++n_out_alleles;
        }
      }
      out->entry_allele_begin[e + 1] = n_out_alleles;
      out->entry_gt_begin[e + 1] = (col0 + ncol) * 2;
    }
    out->site_entry_begin[t + 1] = (t + 1) * nf;
    out->site_stage_status[t] = ragged ? TRGT_MERGE_SITE_RAGGED : 0;
    stats[1] += ragged;
  }
  out->blob_written = blob_at;
  stats[0] = (int64_t)ns; stats[3] = (int64_t)blob_at;
  return TRGT_OK;
}

}  // namespace merge_sites
