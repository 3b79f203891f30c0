// tests/tools/writer_format_check.cpp -- the writer's per-locus formatting (trgt_amd/csrc/writer_format.hpp) held to literal text and
// bytes on batches filled by hand.  The expectations are worked out from the rules of the reference (write_vcf.rs:95-260,
// write_bam.rs:72-144, clip_bases.rs:9-120, tr.rs:196-262) and the BAM specification, not from the code under test.  No GPU, no HIP, no zlib:
//   g++ -std=c++17 -Wall -Werror -I include tests/tools/writer_format_check.cpp -o writer_format_check && ./writer_format_check
// (tests/test_writer_format.py does that).  Exits 0 and ends with "writer_format_check: all held" when everything held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../trgt_amd/csrc/writer_format.hpp"

namespace wf = trgt::wfmt;

static int g_failed = 0;
static std::string g_row;
#define CHECK(cond) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s: %s (line %d)\n", g_row.c_str(), #cond, __LINE__); } } while (0)
static void check_text(const std::string& got, const std::string& want, int line) {
  if (got != want) { ++g_failed; std::printf("FAILED %s (line %d)\n  got  %s\n  want %s\n", g_row.c_str(), line, got.c_str(), want.c_str()); }
}
#define CHECK_TEXT(got, want) check_text(got, want, __LINE__)
static void check_bytes(const std::vector<uint8_t>& got, const std::vector<uint8_t>& want, int line) {
  if (got == want) return;
  ++g_failed;
  size_t i = 0; while (i < got.size() && i < want.size() && got[i] == want[i]) ++i;
  std::printf("FAILED %s (line %d): %zu bytes, want %zu, first difference at %zu\n", g_row.c_str(), line, got.size(), want.size(), i);
}
#define CHECK_BYTES(got, want) check_bytes(got, want, __LINE__)

static const double NaN = std::numeric_limits<double>::quiet_NaN();
constexpr uint32_t M = 0, I = 1, D = 2;  // CIGAR operations
static uint32_t op(uint32_t n, uint32_t c) { return (n << 4) | c; }

// ---------------------------------------------------------------------------------------------------- a batch and its results, by hand
struct Read {
  std::string name, bases; std::vector<uint32_t> cigar; int64_t ref_pos = 0;
  int span_start = -1, span_end = -1, rank = -1, cls = -1;
  bool has_meth = false; std::vector<uint8_t> meth;
  bool reverse = false; uint8_t mapq = 60; int hp = -1; double rq = 0.5; int32_t so = 0, eo = 0; std::vector<int32_t> mo;
};
struct Allele { std::string seq; int lo = 0, hi = 0, sd = 0; std::vector<uint32_t> mc; std::vector<int32_t> spans3; double purity = 1.0; int gt_size = -1; };
struct Locus {
  std::string contig = "chr1", id = "L0", struc = "(CAG)n(CCG)n", lf = "ACGT", tr = "CAGCAG"; std::vector<std::string> motifs = {"CAG", "CCG"};
  int64_t start = 100, end = 106; std::vector<Read> reads; std::vector<Allele> alleles; bool flipped = false;
};
struct Batch {
  trgt_ingest_batch b; trgt_locus_batch_out o;
  std::vector<uint8_t> flank, tr, motif, reads, quals, meth, has_meth, is_reverse, mapq, allele_blob, flipped;
  std::vector<uint64_t> lf_off, tr_off, lrb, read_off, contig_off, id_off, struc_off, name_off, mo_off, meth_off, cigar_off, allele_off, span_off, count_off;
  std::vector<uint32_t> lf_len, tr_len, motif_off, smb, read_len, cigar, allele_len, n_spans, motif_counts;
  std::vector<int64_t> rstart, rend, cigar_ref_pos;
  std::vector<int32_t> so, eo, mo, span_start, span_end, n_alleles, ci, num_spanning, classification, read_rank, spans3, gt_size;
  std::vector<int16_t> hp; std::vector<double> rq, purity;
  std::string contigs, ids, strucs, names;

  explicit Batch(const std::vector<Locus>& loci) {
    motif_off.push_back(0); smb.push_back(0); lrb.push_back(0); contig_off.push_back(0); id_off.push_back(0); struc_off.push_back(0);
    name_off.push_back(0); mo_off.push_back(0); meth_off.push_back(0); cigar_off.push_back(0);
    for (const Locus& L : loci) {
      lf_off.push_back(flank.size()); lf_len.push_back((uint32_t)L.lf.size()); flank.insert(flank.end(), L.lf.begin(), L.lf.end());
      tr_off.push_back(tr.size()); tr_len.push_back((uint32_t)L.tr.size()); tr.insert(tr.end(), L.tr.begin(), L.tr.end());
      for (const std::string& m : L.motifs) { motif.insert(motif.end(), m.begin(), m.end()); motif_off.push_back((uint32_t)motif.size()); }
      smb.push_back((uint32_t)motif_off.size() - 1);
      contigs += L.contig; contig_off.push_back(contigs.size()); ids += L.id; id_off.push_back(ids.size()); strucs += L.struc; struc_off.push_back(strucs.size());
      rstart.push_back(L.start); rend.push_back(L.end);
      for (const Read& R : L.reads) {
        read_off.push_back(reads.size()); read_len.push_back((uint32_t)R.bases.size()); reads.insert(reads.end(), R.bases.begin(), R.bases.end());
        for (size_t i = 0; i < R.bases.size(); ++i) quals.push_back((uint8_t)i);  // the quality of a base is its position in the read
        names += R.name; name_off.push_back(names.size());
        cigar.insert(cigar.end(), R.cigar.begin(), R.cigar.end()); cigar_off.push_back(cigar.size()); cigar_ref_pos.push_back(R.ref_pos);
        has_meth.push_back(R.has_meth); meth.insert(meth.end(), R.meth.begin(), R.meth.end()); meth_off.push_back(meth.size());
        is_reverse.push_back(R.reverse); mapq.push_back(R.mapq); hp.push_back((int16_t)R.hp); rq.push_back(R.rq); so.push_back(R.so); eo.push_back(R.eo);
        mo.insert(mo.end(), R.mo.begin(), R.mo.end()); mo_off.push_back(mo.size());
        span_start.push_back(R.span_start); span_end.push_back(R.span_end); read_rank.push_back(R.rank); classification.push_back(R.cls);
      }
      lrb.push_back(read_off.size());
      n_alleles.push_back((int32_t)L.alleles.size()); flipped.push_back(L.flipped);
      for (int a = 0; a < 2; ++a) {
        const Allele A = a < (int)L.alleles.size() ? L.alleles[(size_t)a] : Allele();
        allele_off.push_back(allele_blob.size()); allele_len.push_back((uint32_t)A.seq.size()); allele_blob.insert(allele_blob.end(), A.seq.begin(), A.seq.end());
        ci.push_back(A.lo); ci.push_back(A.hi); num_spanning.push_back(A.sd); purity.push_back(A.purity); gt_size.push_back(A.gt_size >= 0 ? A.gt_size : (int)A.seq.size());
        span_off.push_back(spans3.size() / 3); n_spans.push_back((uint32_t)A.spans3.size() / 3); spans3.insert(spans3.end(), A.spans3.begin(), A.spans3.end());
        count_off.push_back(motif_counts.size()); motif_counts.insert(motif_counts.end(), A.mc.begin(), A.mc.end()); motif_counts.resize(count_off.back() + L.motifs.size());
      }
    }
    // (a vector that stayed empty must still give a pointer: the writer requires the result arrays)
    for (auto* v : {&reads, &quals, &meth, &has_meth, &is_reverse, &mapq, &allele_blob}) v->push_back(0);
    cigar.push_back(0); mo.push_back(0); spans3.push_back(0); motif_counts.push_back(0); hp.push_back(0); rq.push_back(0); so.push_back(0); eo.push_back(0); cigar_ref_pos.push_back(0);
    span_start.push_back(0); span_end.push_back(0); read_rank.push_back(-1); classification.push_back(0); read_off.push_back(0); read_len.push_back(0);
    std::memset(&b, 0, sizeof b); std::memset(&o, 0, sizeof o);
    b.n_loci = (int64_t)loci.size(); b.n_reads = (int64_t)lrb.back();
    b.flank_blob = flank.data(); b.lf_off = lf_off.data(); b.lf_len = lf_len.data(); b.tr_blob = tr.data(); b.tr_off = tr_off.data(); b.tr_len = tr_len.data();
    b.motif_blob = motif.data(); b.motif_off = motif_off.data(); b.set_motif_begin = smb.data(); b.locus_read_begin = lrb.data();
    b.read_blob = reads.data(); b.read_off = read_off.data(); b.read_len = read_len.data(); b.read_qual = rq.data(); b.qual_blob = quals.data();
    b.contig_blob = contigs.data(); b.contig_off = contig_off.data(); b.id_blob = ids.data(); b.id_off = id_off.data(); b.struc_blob = strucs.data(); b.struc_off = struc_off.data();
    b.region_start = rstart.data(); b.region_end = rend.data(); b.name_blob = names.data(); b.name_off = name_off.data();
    b.is_reverse = is_reverse.data(); b.mapq = mapq.data(); b.hp_tag = hp.data(); b.start_offset = so.data(); b.end_offset = eo.data();
    b.mismatch_offsets = mo.data(); b.mismatch_off = mo_off.data(); b.meth = meth.data(); b.meth_off = meth_off.data(); b.has_meth = has_meth.data();
    b.cigar = cigar.data(); b.cigar_off = cigar_off.data(); b.cigar_ref_pos = cigar_ref_pos.data(); b.read_blob_device = -1;
    o.span_start = span_start.data(); o.span_end = span_end.data(); o.n_alleles = n_alleles.data(); o.allele_blob = allele_blob.data(); o.allele_off = allele_off.data();
    o.allele_len = allele_len.data(); o.ci = ci.data(); o.num_spanning = num_spanning.data(); o.classification = classification.data(); o.read_rank = read_rank.data();
    o.spans3 = spans3.data(); o.span_off = span_off.data(); o.n_spans = n_spans.data(); o.motif_counts = motif_counts.data(); o.count_off = count_off.data();
    o.purity = purity.data(); o.gt_size = gt_size.data(); o.flipped = flipped.data();
  }
  Batch(const Batch&) = delete;
};

static const std::vector<std::string> CONTIGS = {"chr0", "chr1"};
static wf::FormatCtx ctx_of(const Batch& B, int32_t flank_len = 2, bool keep_unmapped = true) {
  wf::FormatCtx c;
  c.b = &B.b; c.o = &B.o; c.contigs = &CONTIGS; c.flank_len = flank_len; c.keep_unmapped = keep_unmapped; c.has_bam = true; c.host_records = true;
  return c;
}
struct Formatted { bool ok; std::string lines, err; std::vector<uint8_t> recs; };
static Formatted format(const wf::FormatCtx& c, int64_t l) {
  Formatted f; std::vector<uint8_t> rec;
  f.ok = wf::format_locus(c, l, f.lines, f.recs, rec, f.err);
  return f;
}
// the sample column of the one VCF line in `lines`, split at ':'
static std::vector<std::string> sample(const std::string& lines) {
  std::vector<std::string> out;
  if (lines.empty() || lines.back() != '\n') return out;
  const size_t tab = lines.rfind('\t');
  std::string s = lines.substr(tab + 1, lines.size() - tab - 2), cur;
  for (char ch : s) { if (ch == ':') { out.push_back(cur); cur.clear(); } else cur += ch; }
  out.push_back(cur);
  return out;
}
static std::string column(const std::string& line, int k) {
  size_t at = 0;
  for (int i = 0; i < k; ++i) at = line.find('\t', at) + 1;
  return line.substr(at, line.find_first_of("\t\n", at) - at);
}

// ---- the canonical locus: one allele, one kept read that carries every tag
// read r1: 10 bases, CpGs at 1 and 5 with calls 10 and 20; span [3, 6), two bases of flank -> the record keeps [1, 8) = CGTACGT, 7 bases
static Read read_r1() {
  Read R; R.name = "r1"; R.bases = "ACGTACGTAC"; R.cigar = {op(10, M)}; R.ref_pos = 1000; R.span_start = 3; R.span_end = 6; R.rank = 0; R.cls = 1;
  R.has_meth = true; R.meth = {10, 20}; R.reverse = true; R.mapq = 37; R.hp = 2; R.rq = 0.5; R.so = -3; R.eo = 4; R.mo = {5, -1};
  return R;
}
static Allele allele(const std::string& seq, int lo, int hi, int sd = 1) { Allele A; A.seq = seq; A.lo = lo; A.hi = hi; A.sd = sd; A.mc = {(uint32_t)seq.size() / 3, 0}; A.spans3 = {0, 0, (int32_t)seq.size()}; return A; }
static Locus locus0() { Locus L; L.reads = {read_r1()}; L.alleles = {allele("CAG", 3, 3)}; L.alleles[0].purity = 0.5; return L; }
static const char* LINE0 = "chr1\t100\t.\tTCAGCAG\tTCAG\t.\t.\tTRID=L0;END=106;MOTIFS=CAG,CCG;STRUC=(CAG)n(CCG)n\tGT:AL:ALLR:SD:MC:MS:AP:AM\t1:3:3-3:1:1_0:0(0-3):0.500000:0.08\n";
// the record of r1 by the BAM specification: 32 bytes of head (refID 1, pos 1001, l_read_name 3, mapq 37, bin 4681, one operation, flag
// reverse | unmapped, l_seq 7, no mate), name, 7M, CGTACGT in nibbles with a zero last nibble, qualities 1 .. 7, then the tags
static const std::vector<uint8_t> REC0 = {
    130, 0, 0, 0, 1, 0, 0, 0, 0xE9, 0x03, 0, 0, 3, 37, 0x49, 0x12, 1, 0, 0x14, 0, 7, 0, 0, 0, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0,
    'r', '1', 0, 0x70, 0, 0, 0, 0x24, 0x81, 0x24, 0x80, 1, 2, 3, 4, 5, 6, 7,
    'T', 'R', 'Z', 'L', '0', 0, 'r', 'q', 'f', 0, 0, 0, 0x3F, 'M', 'C', 'B', 'C', 2, 0, 0, 0, 10, 20,
    'M', 'O', 'B', 'i', 2, 0, 0, 0, 5, 0, 0, 0, 0xFF, 0xFF, 0xFF, 0xFF, 'H', 'P', 'C', 2, 'S', 'O', 'i', 0xFD, 0xFF, 0xFF, 0xFF, 'E', 'O', 'i', 4, 0, 0, 0,
    'A', 'L', 'i', 1, 0, 0, 0, 'F', 'L', 'B', 'I', 2, 0, 0, 0, 2, 0, 0, 0, 2, 0, 0, 0};

static bool holds(const std::vector<uint8_t>& v, const char* tag3) {
  for (size_t i = 0; i + 3 <= v.size(); ++i) if (std::memcmp(v.data() + i, tag3, 3) == 0) return true;
  return false;
}

static void check_set_gt() {
  const std::string tr = "CAGCAG", x = "CAG", y = "CAGCAGCAG";
  struct Row { const char* name; std::vector<std::string> al; const char* gt; std::vector<std::string> alts; };
  const Row rows[] = {{"ref/ref", {tr, tr}, "0/0", {}}, {"ref/alt", {tr, x}, "0/1", {x}}, {"alt/ref", {x, tr}, "1/0", {x}}, {"alt/alt equal", {x, x}, "1/1", {x}},
                      {"alt/alt different", {x, y}, "1/2", {x, y}}, {"haploid ref", {tr}, "0", {}}, {"haploid alt", {y}, "1", {y}}};
  for (const Row& r : rows) {
    g_row = std::string("set_gt ") + r.name;
    std::string al[2], gt; const std::string* alts[2] = {nullptr, nullptr};
    for (size_t a = 0; a < r.al.size(); ++a) al[a] = r.al[a];
    const int n = wf::set_gt(tr, al, (int)r.al.size(), gt, alts);
    CHECK_TEXT(gt, r.gt);
    CHECK(n == (int)r.alts.size());
    for (int s = 0; s < n && s < (int)r.alts.size(); ++s) CHECK_TEXT(*alts[s], r.alts[(size_t)s]);
  }
  // ... and on the line: REF and ALT carry the padding base, ALT is "." without an alternative allele
  g_row = "vcf_line 1/2";
  Locus L; L.alleles = {allele(x, 3, 3, 4), allele(y, 8, 10, 5)};
  L.alleles[0].purity = 0.5; L.alleles[1].purity = NaN; L.alleles[1].mc = {2, 1}; L.alleles[1].spans3 = {};
  L.alleles[0].spans3 = {0, 0, 3, 1, 3, 3};
  Batch B({L});
  CHECK_TEXT(format(ctx_of(B), 0).lines, "chr1\t100\t.\tTCAGCAG\tTCAG,TCAGCAGCAG\t.\t.\tTRID=L0;END=106;MOTIFS=CAG,CCG;STRUC=(CAG)n(CCG)n\tGT:AL:ALLR:SD:MC:MS:AP:AM\t1/2:3,9:3-3,8-10:4,5:1_0,2_1:0(0-3)_1(3-3),.:0.500000,.:.,.\n");
  g_row = "vcf_line 0/0";
  Locus L2; L2.alleles = {allele(tr, 6, 6), allele(tr, 6, 6)};
  Batch B2({L2});
  const Formatted f = format(ctx_of(B2), 0);
  CHECK_TEXT(column(f.lines, 3), "TCAGCAG"); CHECK_TEXT(column(f.lines, 4), "."); CHECK_TEXT(sample(f.lines).at(0), "0/0");
}

static void check_fields() {
  g_row = "missing record, POS of region_start 0";
  Locus L; L.start = 0; L.end = 6;
  Batch B({L});
  CHECK_TEXT(format(ctx_of(B), 0).lines, "chr1\t1\t.\tTCAGCAG\t.\t.\t.\tTRID=L0;END=6;MOTIFS=CAG,CCG;STRUC=(CAG)n(CCG)n\tGT:AL:ALLR:SD:MC:MS:AP:AM\t.:.:.:.:.:.:.:.\n");
  g_row = "POS of region_start 1";
  L.start = 1;
  Batch B1({L});
  CHECK_TEXT(column(format(ctx_of(B1), 0).lines, 1), "1");
  g_row = "the canonical line";  // MS with one span, MC joined with '_', AP %.6f
  Batch B0({locus0()});
  CHECK_TEXT(format(ctx_of(B0), 0).lines, LINE0);
  g_row = "AP rounds to six places";
  Locus L3 = locus0(); L3.alleles[0].purity = 0.12345678; L3.alleles[0].spans3 = {};
  Batch B3({L3});
  const std::vector<std::string> s = sample(format(ctx_of(B3), 0).lines);
  CHECK(s.size() == 8); CHECK_TEXT(s.at(5), "."); CHECK_TEXT(s.at(6), "0.123457");
}

// reads for the AM field: CpGs at 2, 6 and 10
static Read meth_read(const char* name, int rank, int s, int e, std::vector<uint8_t> calls) {
  Read R; R.name = name; R.bases = "AACGTTCGAACGTTAAAAAAAAAA"; R.cigar = {op(24, M)}; R.span_start = s; R.span_end = e; R.rank = rank; R.cls = 0; R.has_meth = true; R.meth = calls;
  return R;
}
static std::string am_of(const Locus& L, bool with_gt_size = true, const double* given = nullptr, std::string* err = nullptr) {
  Batch B({L});
  if (!with_gt_size) B.o.gt_size = nullptr;
  wf::FormatCtx c = ctx_of(B); c.has_bam = false; c.given_meth = given;
  const Formatted f = format(c, 0);
  if (err) *err = f.err;
  if (!f.ok) { CHECK(f.lines.empty()); return "<failed>"; }
  const std::vector<std::string> s = sample(f.lines);
  return s.size() == 8 ? s[7] : "<no sample column>";
}
static void check_am() {
  g_row = "AM one allele";  // the mean over reads of the mean over the CpGs inside the span of call / 255
  Locus L; L.alleles = {allele("CAG", 0, 100)};
  L.reads = {meth_read("a", 0, 2, 11, {255, 0, 51}), meth_read("b", 1, 0, 7, {255, 255, 0})};  // 0.4 and 1.0
  CHECK_TEXT(am_of(L), "0.70");
  g_row = "AM no CpG inside the span, no methylation";
  L.reads = {meth_read("a", 0, 3, 6, {255, 0, 51}), meth_read("b", 1, 2, 11, {})};
  L.reads[1].has_meth = false;
  CHECK_TEXT(am_of(L), ".");
  g_row = "AM nearer size inside the interval";
  Locus T; T.alleles = {allele("CAGCAA", 5, 7), allele("CAGCAGCAGCAA", 10, 13)};
  T.reads = {meth_read("six", 1, 2, 8, {255, 255, 0}), meth_read("twelve", 0, 0, 12, {0, 0, 0}), meth_read("nine", 2, 2, 11, {255, 255, 255})};  // (nine: as far from one size as from the other)
  CHECK_TEXT(am_of(T), "1.00,0.00");
  g_row = "AM a read outside both intervals is dropped";
  T.reads = {meth_read("twenty", 0, 2, 22, {255, 255, 255})};
  CHECK_TEXT(am_of(T), ".,.");
  g_row = "AM nearer size, but outside its interval";
  T.alleles[0].lo = 7; T.reads = {meth_read("six", 0, 2, 8, {255, 255, 0})};
  CHECK_TEXT(am_of(T), ".,.");
  g_row = "AM equal sizes credit both";
  Locus E; E.alleles = {allele("CAGCAGCA", 8, 8), allele("CAGCAGCT", 9, 9)};   // (only the first allele's interval is asked)
  E.reads = {meth_read("eight", 0, 2, 10, {255, 0, 0})};
  CHECK_TEXT(am_of(E), "0.50,0.50");
  g_row = "AM equal distances, different sizes: neither";
  Locus Q; Q.alleles = {allele("CAGCAG", 0, 100), allele("CAGCAGCAGC", 0, 100)};
  Q.reads = {meth_read("eight", 0, 2, 10, {255, 0, 0})};
  CHECK_TEXT(am_of(Q), ".,.");
  g_row = "AM flipped";  // the genotype's first allele is the one output slot 1 shows: its interval (9, 9) does not hold the read
  E.flipped = true;
  CHECK_TEXT(am_of(E), ".,.");
  E.alleles[0].lo = E.alleles[0].hi = 9; E.alleles[1].lo = E.alleles[1].hi = 8;
  CHECK_TEXT(am_of(E), "0.50,0.50");
  T.alleles[0].lo = 5; T.flipped = true; T.reads = {meth_read("six", 0, 2, 8, {255, 255, 0})};  // (a level stays with its allele's output slot)
  CHECK_TEXT(am_of(T), "1.00,.");
  g_row = "AM gt_size, and allele_len without it";
  Locus G; G.alleles = {allele("CAGCAA", 0, 100), allele("CAGCAGCAGCAA", 0, 100)};
  G.alleles[0].gt_size = 12; G.alleles[1].gt_size = 6;
  G.reads = {meth_read("six", 0, 2, 8, {255, 255, 0})};
  CHECK_TEXT(am_of(G), ".,1.00");
  CHECK_TEXT(am_of(G, false), "1.00,.");
  g_row = "AM given";
  const double given[2] = {0.777, NaN};
  CHECK_TEXT(am_of(G, true, given), "0.78,.");
  g_row = "AM malformed profile";
  std::string err;
  L.reads = {meth_read("short_profile", 0, 2, 11, {255})};
  CHECK_TEXT(am_of(L, true, nullptr, &err), "<failed>");
  CHECK_TEXT(err, "Read short_profile has malformed methylation profile");
  L.reads = {meth_read("short_profile", 0, 2, 11, {255})};   // ... which the given values never look at
  const double one[2] = {0.5, NaN};
  CHECK_TEXT(am_of(L, true, one), "0.50");
  L.reads = {meth_read("enough_inside", 0, 2, 7, {255, 0})};  // calls missing only behind the span are not asked for
  CHECK_TEXT(am_of(L), "0.50");
}

static std::vector<uint8_t> record_of(const Read& R, int32_t flank_len = 2, bool keep_unmapped = true, bool* ok = nullptr, std::string* err = nullptr) {
  Locus L = locus0(); L.reads = {R};
  Batch B({L});
  const Formatted f = format(ctx_of(B, flank_len, keep_unmapped), 0);
  if (ok) *ok = f.ok;
  if (err) *err = f.err;
  return f.recs;
}
static void check_records() {
  g_row = "record r1";  // odd length: the last nibble is 0; block_size = the bytes behind it
  CHECK_BYTES(record_of(read_r1()), REC0);
  g_row = "record skip rules";
  bool ok = false; std::string err;
  Read R = read_r1(); R.span_start = 1;                       // span_start < F
  CHECK(record_of(R, 2, true, &ok, &err).empty() && ok && err.empty());
  R = read_r1(); R.span_end = 9;                              // read_len < span_end + F
  CHECK(record_of(R, 2, true, &ok, &err).empty() && ok && err.empty());
  R = read_r1(); R.span_start = R.span_end = 4;               // no flanks, an empty span: clip_bases keeps nothing
  CHECK(record_of(R, 0, true, &ok, &err).empty() && ok && err.empty());
  R = read_r1(); R.span_start = R.span_end = 4;               // (with flanks the same span gives four bases)
  CHECK(record_of(R, 2, true, &ok, &err).size() > 36 && ok);
  g_row = "record without HP, rq, methylation; forward, unmapped flag cleared";
  R = read_r1(); R.hp = -1; R.rq = NaN; R.has_meth = false; R.meth.clear(); R.reverse = false;
  std::vector<uint8_t> want = REC0, got = record_of(R, 2, false);
  want.erase(want.begin() + 67, want.begin() + 77);            // MC:B:C (10 bytes)
  want.erase(want.begin() + 83, want.begin() + 87);            // HP:C (4 bytes, 16 behind MC)
  want[0] = 130 - 14; want[18] = 0; want[63] = 0; want[64] = 0; want[65] = 0x80; want[66] = 0xBF;  // flag 0; rq -1.0f
  CHECK_BYTES(got, want);
  CHECK(!holds(got, "HPC") && !holds(got, "MCB") && holds(REC0, "HPC") && holds(REC0, "MCB"));
  g_row = "record flag bits";
  R = read_r1(); R.reverse = false;
  CHECK(record_of(R, 2, true).at(18) == 0x04 && record_of(read_r1(), 2, false).at(18) == 0x10);
  g_row = "record MC keeps the CpGs whose C stays";  // flank 0: [3, 6) holds the C at 5 only
  R = read_r1();
  got = record_of(R, 0);
  want = {'M', 'C', 'B', 'C', 1, 0, 0, 0, 20};
  CHECK(got.size() > 70 && got[20] == 3 && std::vector<uint8_t>(got.begin() + 61, got.begin() + 70) == want);  // (head 36, name 3, CIGAR 4, bases 2, qualities 3, TR 6, rq 7)
  g_row = "record without a reference-consuming operation";  // bin of [pos, pos + 1): at a multiple of 16 384 an empty interval would land a level up
  R = read_r1(); R.cigar = {op(10, I)}; R.ref_pos = 16384;
  got = record_of(R);
  CHECK(got.size() == REC0.size() && got[8] == 0 && got[9] == 0x40 && got[14] == 0x4A && got[15] == 0x12 && got[39] == 0x71);
  g_row = "record clipped inside operations";  // 2M 3D 4I 4M from 1000, less 1 and 2 bases: 1M 3D 4I 2M from 1001
  R = read_r1(); R.cigar = {op(2, M), op(3, D), op(4, I), op(4, M)};
  got = record_of(R);
  want = {0x10, 0, 0, 0, 0x32, 0, 0, 0, 0x41, 0, 0, 0, 0x20, 0, 0, 0};
  CHECK(got.size() == REC0.size() + 12 && got[8] == 0xE9 && got[16] == 4 && std::vector<uint8_t>(got.begin() + 39, got.begin() + 55) == want);
  g_row = "record CIGAR shorter than the read";
  R = read_r1(); R.cigar = {op(2, M)};
  CHECK(record_of(R, 2, true, &ok, &err).empty() && !ok); CHECK_TEXT(err, "CIGAR shorter than the read");
  g_row = "record 65 535 operations";  // deletions take no query base: 1M, n x 1D, 6M left of the 7 kept bases
  R = read_r1();
  R.cigar.assign(65533 + 2, op(1, D)); R.cigar.front() = op(2, M); R.cigar.back() = op(8, M);
  got = record_of(R, 2, true, &ok, &err);
  CHECK(ok && got.size() == REC0.size() + 4 * 65534 && got[16] == 0xFF && got[17] == 0xFF);
  R.cigar.assign(65534 + 2, op(1, D)); R.cigar.front() = op(2, M); R.cigar.back() = op(8, M);
  CHECK(record_of(R, 2, true, &ok, &err).empty() && !ok);
  CHECK_TEXT(err, "more than 65535 CIGAR operations in a clipped read (the BAM record would need a CG tag)");
  g_row = "record contig not in the header";
  Locus L = locus0(); L.contig = "chrX";
  Batch B({L});
  const Formatted f = format(ctx_of(B), 0);
  CHECK(!f.ok && f.recs.empty()); CHECK_TEXT(f.err, "contig chrX is not in the BAM header"); CHECK_TEXT(f.lines, std::string("chrX") + (LINE0 + 4));
  g_row = "contig_tid";
  CHECK(wf::contig_tid(CONTIGS, "chr1", 4) == 1 && wf::contig_tid(CONTIGS, "chr0zzz", 4) == 0 && wf::contig_tid(CONTIGS, "chr1", 3) == -1 && wf::contig_tid({}, "chr1", 4) == -1);
  g_row = "records only when the host assembles them";
  Batch B0({locus0()});
  wf::FormatCtx c = ctx_of(B0); c.host_records = false;
  Formatted g = format(c, 0);
  CHECK(g.ok && g.recs.empty()); CHECK_TEXT(g.lines, LINE0);
  c.host_records = true; c.has_bam = false;
  g = format(c, 0);
  CHECK(g.ok && g.recs.empty()); CHECK_TEXT(g.lines, LINE0);
}

// a worker's loop over a range of loci: it stops at the first failing locus, what it formatted before stays
static void check_error_leg() {
  g_row = "format_locus over a range with an empty flank in the middle";
  Locus bad = locus0(); bad.lf = ""; bad.id = "L1";
  Locus last = locus0(); last.id = "L2";
  Batch B({locus0(), bad, last});
  const wf::FormatCtx c = ctx_of(B);
  std::string lines, err; std::vector<uint8_t> recs, rec;
  int64_t l = 0;
  for (; l < 3; ++l) if (!wf::format_locus(c, l, lines, recs, rec, err)) break;
  CHECK(l == 1); CHECK_TEXT(err, "Empty flanks are not allowed"); CHECK_TEXT(lines, LINE0); CHECK_BYTES(recs, REC0);
}

static void check_kept_reads() {
  g_row = "kept_reads";  // ranks out of order and with gaps: a slot no read names holds the locus's first read
  Locus L = locus0();
  const int ranks[5] = {2, -1, 0, 5, -1};
  L.reads.clear();
  for (int i = 0; i < 5; ++i) { Read R = read_r1(); R.name = "k" + std::to_string(i); R.rank = ranks[i]; L.reads.push_back(R); }
  Batch B({locus0(), L});
  std::vector<uint64_t> kept = {99, 98, 97};  // (what the vector held does not show)
  wf::kept_reads(&B.b, &B.o, 1, kept);
  CHECK((kept == std::vector<uint64_t>{3, 1, 1, 1, 1, 4}));
  wf::kept_reads(&B.b, &B.o, 0, kept);
  CHECK((kept == std::vector<uint64_t>{0}));
  Locus none = locus0(); none.reads[0].rank = -1;
  Batch B1({none});
  wf::kept_reads(&B1.b, &B1.o, 0, kept);
  CHECK(kept.empty());
  // the records follow that order
  const Formatted f = format(ctx_of(B), 1);
  std::string names;
  for (size_t at = 0; f.ok && at + 36 < f.recs.size(); at += 4 + (f.recs[at] | (size_t)f.recs[at + 1] << 8)) names += std::string((const char*)&f.recs[at + 36], 2) + " ";
  CHECK_TEXT(names, "k2 k0 k0 k0 k0 k3 ");
}

static void check_helpers() {
  g_row = "reg2bin";  // the bins of the BAM specification's reg2bin
  CHECK(wf::reg2bin(0, 1) == 4681 && wf::reg2bin(16383, 16385) == 585 && wf::reg2bin(1 << 17, (1 << 17) + 1) == 4681 + 8 && wf::reg2bin(0, 1 << 29) == 0);
  g_row = "clip_bases_meth";
  std::vector<uint8_t> m; const uint8_t calls[3] = {7, 8, 9};
  wf::clip_bases_meth((const uint8_t*)"CGACGCG", 7, calls, 3, 1, 1, m);   // C at 0 is clipped, C at 3 stays, C at 5 stays (its G is the clipped base)
  CHECK((m == std::vector<uint8_t>{8, 9}));
  g_row = "put16 / put32";
  std::vector<uint8_t> v; wf::put16(v, 0x1234); wf::put32(v, 0x89ABCDEFu);
  CHECK((v == std::vector<uint8_t>{0x34, 0x12, 0xEF, 0xCD, 0xAB, 0x89}));
}

int main() {
  check_set_gt();
  check_fields();
  check_am();
  check_records();
  check_error_leg();
  check_kept_reads();
  check_helpers();
  if (g_failed) { std::printf("writer_format_check: %d FAILED\n", g_failed); return 1; }
  std::printf("writer_format_check: all held\n");
  return 0;
}
