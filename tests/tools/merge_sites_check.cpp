// tests/tools/merge_sites_check.cpp -- the host side of trgt_merge_sites_batch (trgt_amd/csrc/merge_sites_host.hpp: the checks of a call
// and the host twin) on three literal inputs, every output array allocated at exactly the size the header states, so that the address
// and undefined-behaviour sanitizers of the host compiler see every access.  The expectations are written out by hand from
// src/merge/vcf_processor.rs.  No GPU, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/tools/merge_sites_check.cpp -o merge_sites_check && ./merge_sites_check
// (tests/test_merge_sites_tool.py does that).  Exits 0 and ends with "merge_sites_check: all held" when everything held.
#include <cstdio>
#include <string>
#include <vector>

#include "../../trgt_amd/csrc/merge_sites_host.hpp"

static int g_failed = 0;
static const char* g_case = "";
#define CHECK(cond) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s: %s (line %d)\n", g_case, #cond, __LINE__); } } while (0)

constexpr int32_t VE = INT32_MIN + 1, MI = INT32_MIN;
constexpr uint32_t MF = 0x7F800001u, VF = 0x7F800002u, HALF = 0x3F000000u, ONE = 0x3F800000u;

struct Field { std::vector<uint8_t> width; std::vector<uint64_t> begin{0}; std::vector<uint32_t> values; };

struct Input {
  std::vector<int32_t> n_samples; std::vector<uint8_t> pre_v1, am_is_int, pad_base;
  std::vector<uint64_t> frb{0}, rab{0}, off; std::vector<int64_t> pos; std::vector<uint32_t> len; std::string blob;
  Field f[5];
  void file(int32_t samples, bool pre, bool legacy) { n_samples.push_back(samples); pre_v1.push_back(pre); am_is_int.push_back(legacy); frb.push_back(frb.back()); }
  // a record of the last file; a field is its width and the values of all samples
  void record(int64_t p, uint8_t base, std::vector<std::string> alleles, std::vector<std::pair<uint8_t, std::vector<uint32_t>>> fields) {
    pos.push_back(p); pad_base.push_back(base); ++frb.back();
    for (auto& a : alleles) { blob += "#"; off.push_back(blob.size()); len.push_back((uint32_t)a.size()); blob += a; }
    rab.push_back(off.size());
    for (int k = 0; k < 5; ++k) {
      f[k].width.push_back(fields[(size_t)k].first);
      f[k].values.insert(f[k].values.end(), fields[(size_t)k].second.begin(), fields[(size_t)k].second.end());
      f[k].begin.push_back(f[k].values.size());
    }
  }
  trgt_merge_sites_in abi() const {
    trgt_merge_sites_in in{};
    in.n_files = (int32_t)n_samples.size(); in.n_samples = n_samples.data(); in.pre_v1 = pre_v1.data(); in.am_is_int = am_is_int.data(); in.file_record_begin = frb.data();
    in.pos = pos.data(); in.pad_base = pad_base.data(); in.record_allele_begin = rab.data(); in.allele_off = off.data(); in.allele_len = len.data();
    in.allele_blob = (const uint8_t*)blob.data(); in.blob_len = blob.size();
    trgt_merge_field* fl[5] = {&in.gt, &in.al, &in.sd, &in.ap, &in.am};
    for (int k = 0; k < 5; ++k) { fl[k]->width = f[k].width.data(); fl[k]->begin = f[k].begin.data(); fl[k]->values = f[k].values.data(); }
    return in;
  }
};

struct Output {
  std::vector<int32_t> record_site, site_template, status, entry_record, allele_src, gt, al, sd, sample_src;
  std::vector<int64_t> site_pos; std::vector<uint64_t> seb, eab, egb, off; std::vector<uint32_t> len, ap, am; std::vector<uint8_t> blob;
  trgt_merge_sites_out out{};
  Output(const Input& in, const merge_sites::Plan& p, int64_t cap) {
    const size_t nf = in.n_samples.size(), c = (size_t)cap;
    record_site.resize(p.n_records); site_pos.resize(c); site_template.resize(c); status.resize(c); entry_record.resize(c * nf); seb.resize(c + 1); eab.resize(c * nf + 1);
    egb.resize(c * nf + 1); off.resize(p.n_alleles); len.resize(p.n_alleles); allele_src.resize(p.n_alleles); gt.resize(c * p.S * 2); al.resize(c * p.S * 2); sd.resize(c * p.S * 2);
    ap.resize(c * p.S * 2); am.resize(c * p.S * 2); sample_src.resize(c * p.S); blob.resize(p.blob_need);
    out.cap_sites = cap; out.record_site = record_site.data(); out.site_pos = site_pos.data(); out.site_template = site_template.data(); out.site_stage_status = status.data();
    out.entry_record = entry_record.data(); out.site_entry_begin = seb.data(); out.entry_allele_begin = eab.data(); out.allele_off = off.data(); out.allele_len = len.data();
    out.allele_src = allele_src.data(); out.entry_gt_begin = egb.data(); out.gt = gt.data(); out.allele_blob = blob.data(); out.blob_cap = blob.size(); out.al = al.data(); out.sd = sd.data();
    out.ap = ap.data(); out.am = am.data(); out.sample_src = sample_src.data();
  }
};

// the sizing call, then the call with exactly n_sites
static Output run(const Input& input, int64_t want_sites, int64_t stats[4]) {
  const trgt_merge_sites_in in = input.abi();
  merge_sites::Plan plan;
  std::string err;
  std::vector<int32_t> record_site(input.pos.size());
  trgt_merge_sites_out probe{};
  probe.record_site = record_site.data();
  int rc = merge_sites::validate("check", &in, &probe, &plan, &err);
  CHECK(rc == TRGT_OK);
  rc = merge_sites::run_host(&in, &probe, plan, stats);
  CHECK(rc == (want_sites ? TRGT_ERR_NOMEM : TRGT_OK) && probe.n_sites == want_sites);
  Output o(input, plan, probe.n_sites);
  merge_sites::Plan plan2;
  rc = merge_sites::validate("check", &in, &o.out, &plan2, &err);
  if (rc) std::printf("%s\n", err.c_str());
  CHECK(rc == TRGT_OK);
  if (rc == TRGT_OK) CHECK(merge_sites::run_host(&in, &o.out, plan2, stats) == TRGT_OK);
  return o;
}
static std::string allele(const Output& o, const Input& in, size_t x, bool from_out) {
  const char* b = from_out ? (const char*)o.blob.data() : in.blob.data();
  return std::string(b + o.off[x], o.len[x]);
}
template <typename T> static bool eq(const std::vector<T>& got, std::vector<T> want) { return got == want; }

int main() {
  int64_t stats[4];
  {  // the reference's heap test (:667-723): positions 100, 2000, 50, 99 of files 0, 1, 2, 3; no pre-1.0 file, so no blob is written
    g_case = "heap";
    Input in;
    const int64_t p[4] = {100, 2000, 50, 99};
    for (int i = 0; i < 4; ++i) {
      in.file(1, false, false);
      in.record(p[i], 'N', {"A", "AT"}, {{2, {2, 4}}, {2, {1, 2}}, {1, {9}}, {2, {HALF, ONE}}, {1, {ONE}}});
    }
    Output o = run(in, 4, stats);
    CHECK(eq(o.site_pos, {50, 99, 100, 2000}) && eq(o.site_template, {2, 3, 0, 1}) && eq(o.record_site, {2, 3, 0, 1}));
    CHECK(eq(o.entry_record, {-1, -1, 2, -1, -1, -1, -1, 3, 0, -1, -1, -1, -1, 1, -1, -1}));
    CHECK(eq(o.eab, {0, 0, 0, 2, 2, 2, 2, 2, 4, 6, 6, 6, 6, 6, 8, 8, 8}) && eq(o.allele_src, {4, 5, 6, 7, 0, 1, 2, 3}) && o.out.blob_written == 0);
    CHECK(allele(o, in, 1, false) == "AT" && o.off[0] == in.off[4]);
    CHECK(std::vector<int32_t>(o.gt.begin(), o.gt.begin() + 8) == (std::vector<int32_t>{0, VE, 0, VE, 2, 4, 0, VE}));
    CHECK(std::vector<int32_t>(o.sd.begin(), o.sd.begin() + 8) == (std::vector<int32_t>{MI, VE, MI, VE, 9, VE, MI, VE}));
    CHECK(std::vector<uint32_t>(o.am.begin(), o.am.begin() + 8) == (std::vector<uint32_t>{MF, VF, MF, VF, ONE, VF, MF, VF}));
    CHECK(std::vector<int32_t>(o.sample_src.begin(), o.sample_src.begin() + 4) == (std::vector<int32_t>{-1, -1, 2, -1}));
    CHECK(stats[0] == 4 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0);
  }
  {  // a padded and an unpadded file meet; a second record at the position; AL 0 and the haploid zero of a width-2 record are not padded; legacy AM
    g_case = "padding";
    Input in;
    in.file(2, true, true);
    in.record(7, 'g', {"A", "ACC"}, {{2, {2, 4, 2, (uint32_t)VE}}, {2, {3, 5, 3, (uint32_t)VE}}, {1, {1, 2}}, {1, {HALF, ONE}}, {2, {255, 0, (uint32_t)MI, (uint32_t)VE}}});
    in.record(7, 'g', {"C"}, {{1, {2, 2}}, {2, {0, (uint32_t)VE, 4, 4}}, {1, {1, 2}}, {1, {HALF, ONE}}, {1, {128, 16777217}}});
    in.record(9, 'c', {"", "T"}, {{1, {2, 4}}, {2, {0, 9, 4, 4}}, {1, {1, 2}}, {1, {HALF, ONE}}, {1, {(uint32_t)-1, 51}}});
    in.file(1, false, false);
    in.record(7, 'x', {"gA", "gAC", "gACC"}, {{2, {4, 6}}, {2, {2, 3}}, {2, {7, 8}}, {2, {0x7FC00001u, ONE}}, {2, {0xFFFFFFFFu, VF}}});
    Output o = run(in, 3, stats);
    CHECK(eq(o.site_pos, {7, 7, 9}) && eq(o.site_template, {0, 1, 2}) && eq(o.status, {0, 0, 0}) && eq(o.entry_record, {0, 3, 1, -1, 2, -1}));
    CHECK(eq(o.len, {2, 4, 2, 3, 4, 1, 0, 1}) && eq(o.off, {0, 2, 6, 8, 11, 15, 16, 16}) && o.out.blob_written == 17 && stats[2] == 1 && stats[3] == 17);
    CHECK(allele(o, in, 0, true) == "gA" && allele(o, in, 1, true) == "gACC" && allele(o, in, 4, true) == "gACC" && allele(o, in, 5, true) == "C" && allele(o, in, 7, true) == "T");
    CHECK(std::vector<int32_t>(o.gt.begin(), o.gt.begin() + 6) == (std::vector<int32_t>{2, 4, 2, VE, 4, 6}));
    CHECK(std::vector<uint32_t>(o.am.begin(), o.am.begin() + 6) == (std::vector<uint32_t>{ONE, 0u, MF, VF, 0xFFFFFFFFu, VF}));
    CHECK(std::vector<uint32_t>(o.ap.begin(), o.ap.begin() + 6) == (std::vector<uint32_t>{HALF, VF, ONE, VF, 0x7FC00001u, ONE}));
    CHECK(std::vector<uint32_t>(o.am.begin() + 6, o.am.begin() + 12) == (std::vector<uint32_t>{0x3F008081u, VF, 0x47808081u, VF, MF, VF}));   // 128 / 255, 16777216 / 255
    CHECK(o.am[12] == 0xBB808081u && o.am[14] == 0x3E4CCCCDu);                                                                        // -1 / 255, 51 / 255 = 0.2
    CHECK(eq(o.sample_src, {0, 1, 6, 2, 3, -1, 4, 5, -1}) && eq(o.egb, {0, 4, 6, 10, 12, 16, 18}));
  }
  {  // a sample without a value, in GT and in a numeric field; an empty first AL slice in a pre-1.0 file; a file without records; no sites fit 0
    g_case = "ragged";
    Input in;
    in.file(1, true, false);
    in.record(3, 'a', {"A"}, {{1, {2}}, {2, {(uint32_t)VE, 5}}, {1, {1}}, {1, {ONE}}, {1, {ONE}}});
    in.record(4, 'a', {"A"}, {{2, {(uint32_t)VE, (uint32_t)VE}}, {1, {5}}, {1, {1}}, {1, {ONE}}, {1, {ONE}}});
    in.record(5, 'a', {"A"}, {{1, {2}}, {1, {5}}, {1, {1}}, {1, {ONE}}, {2, {VF, ONE}}});
    in.record(6, 'a', {"A"}, {{1, {2}}, {1, {5}}, {1, {1}}, {1, {ONE}}, {1, {ONE}}});
    in.file(3, false, false);
    Output o = run(in, 4, stats);
    CHECK(eq(o.status, {TRGT_MERGE_SITE_RAGGED, TRGT_MERGE_SITE_RAGGED, TRGT_MERGE_SITE_RAGGED, 0}) && stats[1] == 3 && stats[2] == 3);
    CHECK(eq(o.len, {1, 2, 2, 2}) && allele(o, in, 3, true) == "aA" && eq(o.entry_record, {0, -1, 1, -1, 2, -1, 3, -1}));
    Input none;
    none.file(2, true, true);
    Output z = run(none, 0, stats);
    CHECK(z.out.n_sites == 0 && stats[0] == 0);
    // the checks of a call: the first offender is named
    trgt_merge_sites_in bad = in.abi();
    std::vector<int64_t> pos = in.pos;
    pos[2] = 1;
    bad.pos = pos.data();
    merge_sites::Plan plan;
    std::string err;
    CHECK(merge_sites::validate("check", &bad, &o.out, &plan, &err) == TRGT_ERR_INVALID && err.find("pos[2]") != std::string::npos);
    std::vector<uint8_t> width = in.f[3].width;
    width[1] = 3;
    bad = in.abi();
    bad.ap.width = width.data();
    CHECK(merge_sites::validate("check", &bad, &o.out, &plan, &err) == TRGT_ERR_UNSUPPORTED && err.find("ap.width[1]") != std::string::npos);
  }
  if (g_failed) { std::printf("merge_sites_check: %d FAILED\n", g_failed); return 1; }
  std::printf("merge_sites_check: all held\n");
  return 0;
}
