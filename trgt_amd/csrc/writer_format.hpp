// trgt_amd/csrc/writer_format.hpp -- what the writer (writers.hip) formats per locus, as plain functions over a batch of the native
// ingestion and the result arrays of trgt_locus_batch: they append to buffers the caller owns and touch neither a file nor the device.
//   VcfWriter::write / set_gt / encode_*                  src/trgt/writers/write_vcf.rs:95-260
//   BamWriter::write                                      src/trgt/writers/write_bam.rs:72-144
//   HiFiRead::clip_bases                                  src/trgt/reads/clip_bases.rs:9-120
//   get_meth / assign_read / get_tr_meth                  src/trgt/workflows/tr.rs:196-262, 363-398 (the AM field)
// Standard library and the C header only (no HIP, no zlib): tests/tools/writer_format_check.cpp holds it to literal text and bytes on
// the host compiler.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trgt_hip.h"

namespace trgt {
namespace wfmt {

inline void put32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
inline void put16(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
inline uint32_t qlen_of(uint32_t op) { const uint32_t c = op & 0xF; return (c == 0 || c == 1 || c == 4 || c == 7 || c == 8) ? op >> 4 : 0; }
inline uint32_t rlen_of(uint32_t op) { const uint32_t c = op & 0xF; return (c == 0 || c == 2 || c == 3 || c == 7 || c == 8) ? op >> 4 : 0; }
// clip_cigar of HiFiRead::clip_bases (clip_bases.rs:59-118): the operations left after dropping left / right query bases; ref_pos moves
// past the reference bases the dropped prefix consumed.  false: the CIGAR covers fewer query bases than are clipped.
inline bool clip_bases_cigar(const uint32_t* cg, size_t nc, size_t left, size_t right, std::vector<uint32_t>& ops, int64_t& ref_pos) {
  size_t qsum = 0; for (size_t i = 0; i < nc; ++i) qsum += qlen_of(cg[i]);
  if (qsum < left + right) return false;
  size_t keep = qsum - left - right, left_len = left, i = 0;
  uint32_t cur = nc ? cg[0] : 0; bool have = nc > 0;
  while (left_len != 0 && have) {
    const size_t q = qlen_of(cur);
    if (q > left_len) { const uint32_t rest = (uint32_t)(q - left_len); if (rlen_of(cur)) ref_pos += (int64_t)left_len; cur = (rest << 4) | (cur & 0xF); left_len = 0; }
    else { left_len -= q; ref_pos += rlen_of(cur); ++i; have = i < nc; if (have) cur = cg[i]; }
  }
  while (have && keep != 0) {
    const size_t q = qlen_of(cur);
    if (q > keep) { ops.push_back(((uint32_t)keep << 4) | (cur & 0xF)); keep = 0; }
    else { keep -= q; ops.push_back(cur); ++i; have = i < nc; if (have) cur = cg[i]; }
  }
  return true;
}
// the per-CpG methylation values of the CpGs whose C stays inside [left, n - right) (clip_bases.rs:34-52)
inline void clip_bases_meth(const uint8_t* all, size_t n, const uint8_t* me, size_t nme, size_t left, size_t right, std::vector<uint8_t>& meth) {
  size_t ci = 0;
  for (size_t idx = 0; idx + 1 < n; ++idx) if (all[idx] == 'C' && all[idx + 1] == 'G') { if (ci < nme && left <= idx && idx < n - right) meth.push_back(me[ci]); ++ci; }
}

inline int reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
inline uint8_t nib(uint8_t c) { switch (c) { case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
                                             case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14; default: return 15; } }

// What format_locus reads besides the locus: the call's arrays and the writer's settings, as plain values
struct FormatCtx {
  const trgt_ingest_batch* b = nullptr; const trgt_locus_batch_out* o = nullptr;
  const double* given_meth = nullptr;  // trgt_writer_write_meth: Allele::meth per output slot, NaN = None, in place of allele_meth_scan
  const std::vector<std::string>* contigs = nullptr;  // the reference sequences of the BAM header, in its order
  int32_t flank_len = 50; bool keep_unmapped = false, has_bam = false;
  bool host_records = true;  // false: the records of this batch are assembled on the device, format_locus gives the VCF line only
};

// The kept spanning reads of locus l in LocusResult.reads order: read_rank[r] is the read's slot; a slot no read names holds the locus's
// first read.  The one statement of the order rule: the VCF's AM field, the host records and the device records' plan all go by it.
inline void kept_reads(const trgt_ingest_batch* b, const trgt_locus_batch_out* o, int64_t l, std::vector<uint64_t>& kept) {
  const uint64_t r0 = b->locus_read_begin[l], r1 = b->locus_read_begin[l + 1];
  kept.clear();
  for (uint64_t r = r0; r < r1; ++r) if (o->read_rank[r] >= 0) { if ((size_t)o->read_rank[r] >= kept.size()) kept.resize((size_t)o->read_rank[r] + 1, r0); kept[(size_t)o->read_rank[r]] = r; }
}
// the contig's index among the BAM header's reference sequences, -1: not there
inline int contig_tid(const std::vector<std::string>& contigs, const char* name, size_t len) {
  for (size_t i = 0; i < contigs.size(); ++i) if (contigs[i].size() == len && std::memcmp(contigs[i].data(), name, len) == 0) return (int)i;
  return -1;
}

// set_gt (write_vcf.rs:219-260): the GT text of the n_al alleles against the reference sequence tr, and the ALT sequences in the order
// their indices were given out (alts[0 .. return value))
inline int set_gt(const std::string& tr, const std::string* al, int n_al, std::string& gt, const std::string* alts[2]) {
  int n_alt = 0;
  for (int a = 0; a < n_al; ++a) {
    int idx;
    if (al[a] == tr) idx = 0;
    else if (n_alt == 0) { idx = 1; alts[n_alt++] = &al[a]; }
    else if (al[0] == al[1]) idx = 1;
    else { idx = 2; alts[n_alt++] = &al[a]; }
    if (a) gt += "/";
    gt += std::to_string(idx);
  }
  return n_alt;
}

// get_meth (tr.rs:196-229) with assign_read (:238-262) over the kept reads, in the genotype's own order (before "reference allele
// first": slot a of sum / n is the allele that output slot `flipped ? 1 - a : a` shows).  false: err names the read whose profile has
// fewer calls than CpGs inside its span.
inline bool allele_meth_scan(const trgt_ingest_batch* b, const trgt_locus_batch_out* o, int64_t l, const std::vector<uint64_t>& kept, int n_al, bool flipped,
                             double meth_sum[2], size_t meth_n[2], std::string& err) {
  meth_sum[0] = meth_sum[1] = 0; meth_n[0] = meth_n[1] = 0;
  if (!b->has_meth || !b->meth || !b->meth_off) return true;
  auto pre = [&](int a) { return flipped ? 1 - a : a; };  // allele of the original order -> output slot
  const size_t sz[2] = {(size_t)(o->gt_size ? o->gt_size[2 * l + pre(0)] : (int32_t)o->allele_len[2 * l + pre(0)]),
                        n_al == 2 ? (size_t)(o->gt_size ? o->gt_size[2 * l + pre(1)] : (int32_t)o->allele_len[2 * l + pre(1)]) : 0};
  for (uint64_t r : kept) {
    if (!b->has_meth[r] || b->meth_off[r + 1] == b->meth_off[r]) continue;
    const size_t s0 = (size_t)o->span_start[r], s1 = (size_t)o->span_end[r];
    const uint8_t* bases = b->read_blob + b->read_off[r]; const size_t n = b->read_len[r];
    const uint8_t* me = b->meth + b->meth_off[r]; const size_t nme = (size_t)(b->meth_off[r + 1] - b->meth_off[r]);
    double total = 0.0; size_t cpg = 0, ci = 0; bool malformed = false;
    for (size_t pos = 0; pos + 1 < n; ++pos)
      if (bases[pos] == 'C' && bases[pos + 1] == 'G') {
        if (s0 <= pos && pos < s1) { if (ci >= nme) { malformed = true; break; } ++cpg; total += (double)me[ci] / 255.0; }
        ++ci;
      }
    if (malformed) { err = "Read " + std::string(b->name_blob + b->name_off[r], b->name_off[r + 1] - b->name_off[r]) + " has malformed methylation profile"; return false; }
    if (!cpg) continue;
    const double level = total / (double)cpg;
    const size_t len = s1 - s0;
    if (n_al == 1) { meth_sum[0] += level; ++meth_n[0]; continue; }  // assign_read (:238-262)
    const auto adiff = [](size_t x, size_t y) { return x > y ? x - y : y - x; };
    const bool sp1 = (size_t)o->ci[4 * l + 2 * pre(0)] <= len && len <= (size_t)o->ci[4 * l + 2 * pre(0) + 1];
    const bool sp2 = (size_t)o->ci[4 * l + 2 * pre(1)] <= len && len <= (size_t)o->ci[4 * l + 2 * pre(1) + 1];
    const size_t d1 = adiff(len, sz[0]), d2 = adiff(len, sz[1]);
    if (d1 < d2 && sp1) { meth_sum[0] += level; ++meth_n[0]; }
    else if (d2 < d1 && sp2) { meth_sum[1] += level; ++meth_n[1]; }
    else if (sz[0] == sz[1] && sp1) { meth_sum[0] += level; ++meth_n[0]; meth_sum[1] += level; ++meth_n[1]; }
  }
  return true;
}

// The sample column behind GT: ":AL:ALLR:SD:MC:MS:AP:AM" of the n_al alleles (encode_*, write_vcf.rs:262-397), appended to line.
// n_motifs: motifs of the locus's set; meth_sum / meth_n: allele_meth_scan's (read only without given_meth).
inline void sample_fields(const trgt_locus_batch_out* o, int64_t l, int n_al, uint32_t n_motifs, bool flipped, const double* given_meth, const double meth_sum[2],
                          const size_t meth_n[2], std::string& line) {
  std::string f_al, f_allr, f_sd, f_mc, f_ms, f_ap, f_am;
  char num[64];
  for (int a = 0; a < n_al; ++a) {
    const char* sep = a ? "," : "";
    f_al += sep; f_al += std::to_string(o->allele_len[2 * l + a]);
    f_allr += sep; f_allr += std::to_string(o->ci[4 * l + 2 * a]) + "-" + std::to_string(o->ci[4 * l + 2 * a + 1]);
    f_sd += sep; f_sd += std::to_string(o->num_spanning[2 * l + a]);
    f_mc += sep;
    for (uint32_t m = 0; m < n_motifs; ++m) { if (m) f_mc += "_"; f_mc += std::to_string(o->motif_counts[o->count_off[2 * l + a] + m]); }
    f_ms += sep;
    const uint32_t ns = o->n_spans[2 * l + a];
    if (ns == 0) f_ms += ".";
    for (uint32_t k = 0; k < ns; ++k) {
      const int32_t* sp = o->spans3 + 3 * (o->span_off[2 * l + a] + k);
      if (k) f_ms += "_";
      f_ms += std::to_string(sp[0]) + "(" + std::to_string(sp[1]) + "-" + std::to_string(sp[2]) + ")";
    }
    f_ap += sep;
    if (std::isnan(o->purity[2 * l + a])) f_ap += "."; else { std::snprintf(num, sizeof num, "%.6f", o->purity[2 * l + a]); f_ap += num; }
    f_am += sep;
    const int src = flipped ? 1 - a : a;  // the allele's slot in the original order
    if (given_meth) { if (std::isnan(given_meth[2 * l + a])) f_am += "."; else { std::snprintf(num, sizeof num, "%.2f", given_meth[2 * l + a]); f_am += num; } }
    else if (meth_n[src]) { std::snprintf(num, sizeof num, "%.2f", meth_sum[src] / (double)meth_n[src]); f_am += num; } else f_am += ".";
  }
  line += ":" + f_al + ":" + f_allr + ":" + f_sd + ":" + f_mc + ":" + f_ms + ":" + f_ap + ":" + f_am;
}

// The VCF record of locus l (write_vcf.rs:95-260), appended to lines; kept: kept_reads of the locus.  false: err says why, lines is
// as it was.
inline bool vcf_line(const FormatCtx& c, int64_t l, const std::vector<uint64_t>& kept, std::string& lines, std::string& err) {
  const trgt_ingest_batch* b = c.b; const trgt_locus_batch_out* o = c.o;
  if (b->lf_len[l] == 0) { err = "Empty flanks are not allowed"; return false; }
  const char pad = (char)b->flank_blob[b->lf_off[l] + b->lf_len[l] - 1];
  const std::string tr((const char*)b->tr_blob + b->tr_off[l], b->tr_len[l]);
  const int n_al = o->n_alleles[l];
  const uint32_t m0 = b->set_motif_begin[l], m1 = b->set_motif_begin[l + 1];
  const bool flipped = o->flipped && o->flipped[l] && n_al == 2;
  double meth_sum[2] = {0, 0}; size_t meth_n[2] = {0, 0};
  if (n_al != 0 && !c.given_meth && !allele_meth_scan(b, o, l, kept, n_al, flipped, meth_sum, meth_n, err)) return false;
  std::string line;
  line.append(b->contig_blob + b->contig_off[l], b->contig_off[l + 1] - b->contig_off[l]);
  line += '\t'; line += std::to_string(b->region_start[l] > 0 ? b->region_start[l] : 1); line += "\t.\t";  // POS = saturating_sub(start, 1) + 1
  std::string info = "TRID="; info.append(b->id_blob + b->id_off[l], b->id_off[l + 1] - b->id_off[l]);
  info += ";END=" + std::to_string(b->region_end[l]) + ";MOTIFS=";
  for (uint32_t m = m0; m < m1; ++m) { if (m > m0) info += ","; info.append((const char*)b->motif_blob + b->motif_off[m], b->motif_off[m + 1] - b->motif_off[m]); }
  info += ";STRUC="; info.append(b->struc_blob + b->struc_off[l], b->struc_off[l + 1] - b->struc_off[l]);
  line += pad; line += tr; line += '\t';
  if (n_al == 0) {  // add_missing_allele_info
    line += ".\t.\t.\t"; line += info; line += "\tGT:AL:ALLR:SD:MC:MS:AP:AM\t.:.:.:.:.:.:.:.\n";
  } else {
    std::string al[2], gt;
    for (int a = 0; a < n_al; ++a) al[a].assign((const char*)o->allele_blob + o->allele_off[2 * l + a], o->allele_len[2 * l + a]);
    const std::string* alts[2];
    const int n_alt = set_gt(tr, al, n_al, gt, alts);
    if (n_alt == 0) line += ".";
    for (int s = 0; s < n_alt; ++s) { if (s) line += ","; line += pad; line += *alts[s]; }
    line += "\t.\t.\t"; line += info; line += "\tGT:AL:ALLR:SD:MC:MS:AP:AM\t"; line += gt;
    sample_fields(o, l, n_al, m1 - m0, flipped, c.given_meth, meth_sum, meth_n, line);
    line += "\n";
  }
  lines += line;
  return true;
}

// One kept read r of locus l as a spanning-BAM record (write_bam.rs:72-144) in rec, block_size word included.  tid: the locus's contig
// in the header; id: the locus id (TR:Z).  REC_SKIPPED: the read's span leaves it fewer than flank_len bases on a side, or clip_bases
// keeps nothing -- no record, no error.
enum RecResult { REC_SKIPPED = 0, REC_WRITTEN = 1, REC_ERROR = 2 };
inline RecResult bam_record(const FormatCtx& c, uint64_t r, int tid, const char* id, size_t id_len, std::vector<uint8_t>& rec, std::string& err) {
  const trgt_ingest_batch* b = c.b; const trgt_locus_batch_out* o = c.o;
  const size_t F = (size_t)c.flank_len;
  const size_t s0 = (size_t)o->span_start[r], s1 = (size_t)o->span_end[r], n = b->read_len[r];
  if (s0 < F || n < s1 + F) return REC_SKIPPED;  // "unexpectedly short flanks"
  const size_t left = s0 - F, right = n - s1 - F;
  if (left + right >= n) return REC_SKIPPED;     // clip_bases: None
  const uint8_t* bases = b->read_blob + b->read_off[r] + left; const uint8_t* quals = b->qual_blob + b->read_off[r] + left;
  const size_t len = n - left - right;
  std::vector<uint32_t> ops; int64_t ref_pos = b->cigar_ref_pos[r];
  if (!clip_bases_cigar(b->cigar + b->cigar_off[r], (size_t)(b->cigar_off[r + 1] - b->cigar_off[r]), left, right, ops, ref_pos)) { err = "CIGAR shorter than the read"; return REC_ERROR; }
  if (ops.size() > 65535) { err = "more than 65535 CIGAR operations in a clipped read (the BAM record would need a CG tag)"; return REC_ERROR; }
  std::vector<uint8_t> meth; bool has_meth = false;
  if (b->has_meth && b->has_meth[r]) {
    has_meth = true;
    clip_bases_meth(b->read_blob + b->read_off[r], n, b->meth + b->meth_off[r], (size_t)(b->meth_off[r + 1] - b->meth_off[r]), left, right, meth);
  }
  const char* name = b->name_blob + b->name_off[r]; const size_t name_len = (size_t)(b->name_off[r + 1] - b->name_off[r]);
  int64_t ref_end = ref_pos; for (uint32_t op : ops) ref_end += rlen_of(op);
  rec.clear();
  put32(rec, 0);  // block_size, patched below
  put32(rec, (uint32_t)tid); put32(rec, (uint32_t)ref_pos);
  rec.push_back((uint8_t)(name_len + 1)); rec.push_back(b->mapq[r]);
  put16(rec, (uint32_t)reg2bin(ref_pos, ref_end > ref_pos ? ref_end : ref_pos + 1)); put16(rec, (uint32_t)ops.size());
  put16(rec, (b->is_reverse[r] ? 0x10u : 0u) | (c.keep_unmapped ? 0x4u : 0u)); put32(rec, (uint32_t)len);
  put32(rec, 0xFFFFFFFFu); put32(rec, 0xFFFFFFFFu); put32(rec, 0);  // mate: none
  rec.insert(rec.end(), name, name + name_len); rec.push_back(0);
  for (uint32_t op : ops) put32(rec, op);
  for (size_t i = 0; i < len; i += 2) rec.push_back((uint8_t)((nib(bases[i]) << 4) | (i + 1 < len ? nib(bases[i + 1]) : 0)));
  rec.insert(rec.end(), quals, quals + len);
  auto tag = [&](const char* t, char ty) { rec.push_back((uint8_t)t[0]); rec.push_back((uint8_t)t[1]); rec.push_back((uint8_t)ty); };
  tag("TR", 'Z'); rec.insert(rec.end(), id, id + id_len); rec.push_back(0);
  { tag("rq", 'f'); const float f = std::isnan(b->read_qual[r]) ? -1.0f : (float)b->read_qual[r]; uint32_t u; std::memcpy(&u, &f, 4); put32(rec, u); }
  if (has_meth) { tag("MC", 'B'); rec.push_back('C'); put32(rec, (uint32_t)meth.size()); rec.insert(rec.end(), meth.begin(), meth.end()); }
  { tag("MO", 'B'); rec.push_back('i'); const uint64_t a0 = b->mismatch_off[r], a1 = b->mismatch_off[r + 1]; put32(rec, (uint32_t)(a1 - a0)); for (uint64_t k = a0; k < a1; ++k) put32(rec, (uint32_t)b->mismatch_offsets[k]); }
  if (b->hp_tag[r] >= 0) { tag("HP", 'C'); rec.push_back((uint8_t)b->hp_tag[r]); }
  tag("SO", 'i'); put32(rec, (uint32_t)b->start_offset[r]);
  tag("EO", 'i'); put32(rec, (uint32_t)b->end_offset[r]);
  tag("AL", 'i'); put32(rec, (uint32_t)o->classification[r]);
  tag("FL", 'B'); rec.push_back('I'); put32(rec, 2); put32(rec, (uint32_t)F); put32(rec, (uint32_t)F);
  const uint32_t bs = (uint32_t)rec.size() - 4;
  for (int i = 0; i < 4; ++i) rec[(size_t)i] = (uint8_t)(bs >> (8 * i));
  return REC_WRITTEN;
}

// One locus: its VCF line and -- when the host assembles them -- its spanning-BAM records, appended to the caller's buffers (loci are
// independent: a batch is formatted by several workers over contiguous ranges of loci, and the pieces are written in locus order).
// rec: scratch for one record.  false: err says why; the line and the records in front of the failing one stay appended.
inline bool format_locus(const FormatCtx& c, int64_t l, std::string& lines, std::vector<uint8_t>& recs, std::vector<uint8_t>& rec, std::string& err) {
  const trgt_ingest_batch* b = c.b;
  std::vector<uint64_t> kept;
  kept_reads(b, c.o, l, kept);
  if (!vcf_line(c, l, kept, lines, err)) return false;
  if (!c.has_bam || !c.host_records) return true;
  const char* contig = b->contig_blob + b->contig_off[l]; const size_t contig_len = (size_t)(b->contig_off[l + 1] - b->contig_off[l]);
  const int tid = contig_tid(*c.contigs, contig, contig_len);
  if (tid < 0) { err = "contig " + std::string(contig, contig_len) + " is not in the BAM header"; return false; }
  for (uint64_t r : kept) {
    const RecResult res = bam_record(c, r, tid, b->id_blob + b->id_off[l], (size_t)(b->id_off[l + 1] - b->id_off[l]), rec, err);
    if (res == REC_ERROR) return false;
    if (res == REC_WRITTEN) recs.insert(recs.end(), rec.begin(), rec.end());
  }
  return true;
}

}  // namespace wfmt
}  // namespace trgt
