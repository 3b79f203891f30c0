// tests/tools/ingest_plan_check.cpp -- the plan of the device-side read ingestion (trgt_amd/csrc/ingest_plan.hpp) held to literal values worked
// out by hand from its rules: the windows of a locus, the compressed ranges and their place in the staging buffer, the block table read off
// hand-built BGZF headers (arbitrary payload bytes: the walk reads headers and footers only), the chunks as positions in the inflated
// bytes, the slab layout, and the lease of a slab against a pool that counts what it is given.  No GPU, no HIP, no zlib:
//   g++ -std=c++17 -O1 -Wall -Werror tests/tools/ingest_plan_check.cpp -o ingest_plan_check && ./ingest_plan_check
// (tests/test_ingest_plan.py does that; with -fsanitize=address,undefined every byte the walk reads is checked against the staged buffer).
// Exits 0 and ends with "ingest_plan_check: all held" when everything held.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../trgt_amd/csrc/ingest_plan.hpp"

using namespace trgt;
using namespace trgt::ingd;

static int g_failed = 0;
static std::string g_row;
#define CHECK(cond) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s: %s (line %d)\n", g_row.c_str(), #cond, __LINE__); } } while (0)

static VoffPair chunk(uint64_t c0, uint32_t u0, uint64_t c1, uint32_t u1) { return {(c0 << 16) | u0, (c1 << 16) | u1}; }

// ---- windows
static void windows() {
  g_row = "windows";
  const LocusDesc a = locus_windows(3, 100, 160, 250);
  CHECK(a.tid == 3 && a.pad == 0 && a.chunk_begin == 0 && a.chunk_end == 0);
  CHECK(a.beg == 0 && a.end == 410);                        // the fetch window is clamped at 0
  CHECK(a.region_start == 100 && a.region_end == 160);      // the region is as given
  CHECK(a.clip_start == -400 && a.clip_end == 660);         // the clip window is not clamped
  const LocusDesc b = locus_windows(-1, 1000, 1030, 250);
  CHECK(b.tid == -1 && b.beg == 750 && b.end == 1280 && b.clip_start == 500 && b.clip_end == 1530);
  // a locus with tid -1 gets no chunks (and the .bai is not asked); its neighbours get theirs, one after the other
  std::vector<LocusDesc> loci = {a, b, locus_windows(0, 5000, 5010, 10)};
  int asked = 0;
  const std::vector<VoffPair> cv = locus_chunks(loci, [&](int tid, int64_t beg, int64_t end) {
    ++asked;
    CHECK(tid >= 0);
    CHECK((tid == 3 && beg == 0 && end == 410) || (tid == 0 && beg == 4990 && end == 5020));
    return tid == 3 ? std::vector<VoffPair>{chunk(10, 1, 20, 2), chunk(30, 3, 40, 4)} : std::vector<VoffPair>{chunk(50, 5, 60, 6)};
  });
  CHECK(asked == 2 && cv.size() == 3);
  CHECK(loci[0].chunk_begin == 0 && loci[0].chunk_end == 2 && loci[1].chunk_begin == 2 && loci[1].chunk_end == 2 && loci[2].chunk_begin == 2 && loci[2].chunk_end == 3);
  CHECK(cv[1] == chunk(30, 3, 40, 4) && cv[2] == chunk(50, 5, 60, 6));
}

// ---- ranges
static void ranges() {
  const uint64_t big = 1ull << 30;
  g_row = "ranges_gap_0x10000_merges";
  {  // the second chunk's first block starts exactly 0x10000 behind the first chunk's last block (given in the other order: sorted first)
    const RangePlan rp = plan_ranges({chunk(67536, 7, 70000, 9), chunk(1000, 1, 2000, 2)}, big);
    CHECK(rp.ranges.size() == 1 && rp.ranges[0] == VoffPair(1000, 70000));
    CHECK(rp.read_end[0] == 135600 && rp.src_at[0] == 0 && rp.src_total == 134656);  // 134600 bytes, rounded up to 64
    CHECK(rp.pieces.size() == 1 && rp.pieces[0].file_off == 1000 && rp.pieces[0].src_off == 0 && rp.pieces[0].n == 134600);
  }
  g_row = "ranges_gap_0x10001_does_not_merge";
  {
    const RangePlan rp = plan_ranges({chunk(1000, 1, 2000, 2), chunk(67537, 7, 70000, 9)}, big);
    CHECK(rp.ranges.size() == 2 && rp.ranges[0] == VoffPair(1000, 2000) && rp.ranges[1] == VoffPair(67537, 70000));
    CHECK(rp.read_end[0] == 67600 && rp.read_end[1] == 135600);
    CHECK(rp.src_at[0] == 0 && rp.src_at[1] == 66624 && rp.src_total == 134720);  // 66600 -> 66624; 68063 -> 68096
    CHECK(rp.src_at[1] % 64 == 0 && rp.src_total % 64 == 0);
    CHECK(rp.pieces.size() == 2 && rp.pieces[0].file_off == 1000 && rp.pieces[0].src_off == 0 && rp.pieces[0].n == 66600);
    CHECK(rp.pieces[1].file_off == 67537 && rp.pieces[1].src_off == 66624 && rp.pieces[1].n == 68063);
  }
  g_row = "ranges_overlap_keeps_the_larger_end";
  {
    const RangePlan rp = plan_ranges({chunk(1000, 0, 9000, 0), chunk(2000, 0, 3000, 0)}, big);
    CHECK(rp.ranges.size() == 1 && rp.ranges[0] == VoffPair(1000, 9000) && rp.read_end[0] == 74600);
  }
  g_row = "ranges_read_end_clipped_by_fsize";
  {
    const RangePlan rp = plan_ranges({chunk(1000, 1, 2000, 2)}, 5000);
    CHECK(rp.fsize == 5000 && rp.read_end[0] == 5000 && rp.src_total == 4032);  // 4000 -> 4032
    CHECK(rp.pieces.size() == 1 && rp.pieces[0].n == 4000);
  }
  g_row = "ranges_pieces_of_4_mib";
  {  // 4 MiB + 1 byte to read: 100 .. 4128805 + 0x10000 + 64 = 4194405
    const RangePlan rp = plan_ranges({chunk(100, 0, 4128805, 0)}, big);
    CHECK(rp.read_end[0] == 4194405 && rp.src_total == 4194368);
    CHECK(rp.pieces.size() == 2 && rp.pieces[0].file_off == 100 && rp.pieces[0].src_off == 0 && rp.pieces[0].n == 4194304);
    CHECK(rp.pieces[1].file_off == 4194404 && rp.pieces[1].src_off == 4194304 && rp.pieces[1].n == 1);
  }
  g_row = "ranges_no_chunks";
  {
    const RangePlan rp = plan_ranges({}, big);
    CHECK(rp.ranges.empty() && rp.read_end.empty() && rp.src_at.empty() && rp.pieces.empty() && rp.src_total == 0);
    const BlockWalk w = walk_block_headers(nullptr, 0, rp);
    CHECK(w.fallback == FB_NONE && w.blocks.empty() && w.known.empty() && w.infl_bytes == 0);
  }
}

// ---- BGZF blocks by hand: the 12 fixed bytes with FEXTRA, an extra field that holds BC (behind a 7-byte "XY" subfield if asked), payload bytes
// that mean nothing, CRC-32, ISIZE.  `total` is the whole block: header 18 (or 25) + payload + 8.
static std::vector<uint8_t> bgzf_block(uint32_t total, uint32_t isize, uint32_t crc, bool bc_second = false) {
  std::vector<uint8_t> b = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, (uint8_t)(bc_second ? 13 : 6), 0};
  const uint8_t xy[7] = {'X', 'Y', 3, 0, 1, 2, 3};
  if (bc_second) b.insert(b.end(), xy, xy + 7);
  for (uint8_t v : {(uint8_t)'B', (uint8_t)'C', (uint8_t)2, (uint8_t)0, (uint8_t)((total - 1) & 0xFF), (uint8_t)((total - 1) >> 8)}) b.push_back(v);
  while (b.size() + 8 < total) b.push_back(0xAA);
  for (uint32_t v : {crc, isize}) for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(v >> (8 * k)));
  return b;
}
// the staged buffer of a plan: the file's bytes [first, read_end) of every range at its src_at (exactly src_total bytes: a sanitizer build sees
// every byte the walk reads beyond it)
static std::vector<uint8_t> stage(const RangePlan& rp, const std::vector<uint8_t>& file) {
  std::vector<uint8_t> src(rp.src_total, 0);
  for (size_t i = 0; i < rp.ranges.size(); ++i)
    for (uint64_t o = rp.ranges[i].first; o < rp.read_end[i] && o < file.size(); ++o) src[rp.src_at[i] + (o - rp.ranges[i].first)] = file[o];
  return src;
}
static void put(std::vector<uint8_t>& file, uint64_t at, const std::vector<uint8_t>& b) {
  if (file.size() < at + b.size()) file.resize(at + b.size(), 0);
  std::memcpy(file.data() + at, b.data(), b.size());
}
static bool same(const infl::BlockDesc& b, uint64_t src_off, uint64_t dst_off, uint32_t src_len, uint32_t dst_len) {
  return b.src_off == src_off && b.dst_off == dst_off && b.src_len == src_len && b.dst_len == dst_len;
}
static bool same(const KnownBlock& k, uint64_t coff, uint64_t lin, uint32_t isize, uint32_t range) { return k.coff == coff && k.lin == lin && k.isize == isize && k.range == range; }
static bool same(const ChunkDesc& c, uint64_t lin0, uint64_t lin1, uint64_t lin_limit) { return c.lin0 == lin0 && c.lin1 == lin1 && c.lin_limit == lin_limit; }

// The file of the header and chunk rows: A at 0 (100 bytes, inflates to 1000), B at 100 (BC behind another subfield; 60 bytes, 500), an empty
// block E at 160 (28 bytes, the EOF block's shape), C at 188 (50 bytes, 70), D at 238 (40 bytes, 9); far behind, F at 70000 (30 bytes, 40),
// where the file ends.  The chunks end in C, so the first range is [0, 188] and D is never walked.
static void headers_and_chunks() {
  g_row = "headers_two_ranges";
  std::vector<uint8_t> file;
  put(file, 0, bgzf_block(100, 1000, 0x11111111u)); put(file, 100, bgzf_block(60, 500, 0x22222222u, true)); put(file, 160, bgzf_block(28, 0, 0));
  put(file, 188, bgzf_block(50, 70, 0x33333333u)); put(file, 238, bgzf_block(40, 9, 0x44444444u)); put(file, 70000, bgzf_block(30, 40, 0x55555555u));
  CHECK(file.size() == 70030);
  const RangePlan rp = plan_ranges({chunk(0, 5, 188, 10), chunk(70000, 0, 70000, 20)}, file.size());
  CHECK(rp.ranges.size() == 2 && rp.ranges[0] == VoffPair(0, 188) && rp.ranges[1] == VoffPair(70000, 70000));
  CHECK(rp.read_end[0] == 65788 && rp.read_end[1] == 70030 && rp.src_at[1] == 65792 && rp.src_total == 65856);
  const std::vector<uint8_t> src = stage(rp, file);
  const BlockWalk w = walk_block_headers(src.data(), src.size(), rp);
  CHECK(w.fallback == FB_NONE);
  // the block table: the empty block is not in it; the payload of B starts behind its 25-byte header
  CHECK(w.blocks.size() == 4 && w.crcs.size() == 4);
  CHECK(same(w.blocks[0], 18, 0, 74, 1000) && same(w.blocks[1], 125, 1000, 27, 500) && same(w.blocks[2], 206, 1500, 24, 70) && same(w.blocks[3], 65810, 1664, 4, 40));
  CHECK(w.crcs[0] == 0x11111111u && w.crcs[1] == 0x22222222u && w.crcs[2] == 0x33333333u && w.crcs[3] == 0x55555555u);
  // known: the empty block too, advancing nothing; D (beyond the range's last block) is not met; F starts at ((1570 + 63) & ~63) + 64
  CHECK(w.known.size() == 5);
  CHECK(same(w.known[0], 0, 0, 1000, 0) && same(w.known[1], 100, 1000, 500, 0) && same(w.known[2], 160, 1500, 0, 0) && same(w.known[3], 188, 1500, 70, 0) && same(w.known[4], 70000, 1664, 40, 1));
  CHECK(w.lin_end.size() == 2 && w.lin_end[0] == 1570 && w.lin_end[1] == 1704 && w.infl_bytes == 1792);
  g_row = "headers_staged_bytes_shorter_than_the_plan";
  CHECK(walk_block_headers(src.data(), src.size() - 1, rp).fallback == FB_BLOCK);

  std::vector<ChunkDesc> cd;
  g_row = "chunks_placed";
  CHECK(place_chunks({chunk(0, 5, 188, 10), chunk(70000, 0, 70000, 20), chunk(0, 5, 160, 0)}, w, cd) == FB_NONE && cd.size() == 3);
  CHECK(same(cd[0], 5, 1510, 1570) && same(cd[1], 1664, 1684, 1704) && same(cd[2], 5, 1500, 1570));
  g_row = "chunks_start_block_not_known";
  CHECK(place_chunks({chunk(238, 0, 238, 5)}, w, cd) == FB_WALK);     // D was never walked
  CHECK(place_chunks({chunk(50, 0, 100, 5)}, w, cd) == FB_WALK);      // no block starts at 50
  g_row = "chunks_start_offset_against_isize";
  CHECK(place_chunks({chunk(100, 501, 188, 0)}, w, cd) == FB_WALK);   // greater than B's 500
  CHECK(place_chunks({chunk(100, 500, 188, 0)}, w, cd) == FB_NONE && same(cd[0], 1500, 1500, 1570));  // equal: accepted
  g_row = "chunks_end_block";
  CHECK(place_chunks({chunk(0, 5, 238, 3)}, w, cd) == FB_NONE && same(cd[0], 5, 1570, 1570));       // unknown: lin_limit
  CHECK(place_chunks({chunk(0, 5, 70000, 20)}, w, cd) == FB_NONE && same(cd[0], 5, 1570, 1570));    // in the other range: lin_limit
  CHECK(place_chunks({chunk(0, 5, 100, 600)}, w, cd) == FB_NONE && same(cd[0], 5, 1500, 1570));     // 600 > isize 500: clamped to the block's end
  CHECK(place_chunks({}, w, cd) == FB_NONE && cd.empty());
}

// one block at offset 0 of a file of `fsize` bytes (longer than the block: zero bytes follow), chunk 0:0 -> 0:0
static int walk_one(std::vector<uint8_t> block, uint64_t fsize) {
  std::vector<uint8_t> file = block;
  file.resize(fsize, 0);
  const RangePlan rp = plan_ranges({chunk(0, 0, 0, 0)}, fsize);
  const std::vector<uint8_t> src = stage(rp, file);
  const BlockWalk w = walk_block_headers(src.data(), src.size(), rp);
  if (w.fallback) CHECK(w.blocks.empty() && w.known.empty() && w.crcs.empty() && w.infl_bytes == 0);
  return w.fallback;
}
static void refused_headers() {
  g_row = "header_accepted";
  CHECK(walk_one(bgzf_block(100, 1000, 1), 100) == FB_NONE);
  CHECK(walk_one(bgzf_block(100, 1000, 1, true), 200) == FB_NONE);
  CHECK(walk_one(bgzf_block(100, 0x10000, 1), 100) == FB_NONE);
  g_row = "header_fewer_than_18_bytes";
  CHECK(walk_one(bgzf_block(100, 1000, 1), 17) == FB_BLOCK);
  g_row = "header_magic_or_fextra";
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[0] = 30; CHECK(walk_one(b, 100) == FB_BLOCK); }
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[1] = 138; CHECK(walk_one(b, 100) == FB_BLOCK); }
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[2] = 9; CHECK(walk_one(b, 100) == FB_BLOCK); }
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[3] = 0; CHECK(walk_one(b, 100) == FB_BLOCK); }
  g_row = "header_xlen_past_the_end";
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[10] = 100; CHECK(walk_one(b, 100) == FB_BLOCK); }   // 12 + 100 > 100
  g_row = "header_no_bc";
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[13] = 'D'; CHECK(walk_one(b, 100) == FB_BLOCK); }
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[14] = 3; CHECK(walk_one(b, 100) == FB_BLOCK); }     // BC of another length is not BC
  g_row = "header_total_below_header_and_footer";
  { std::vector<uint8_t> b = bgzf_block(100, 1000, 1); b[16] = 24; b[17] = 0; CHECK(walk_one(b, 100) == FB_BLOCK); }  // total 25 < 18 + 8
  { std::vector<uint8_t> b = bgzf_block(26, 0, 0); CHECK(walk_one(b, 26) == FB_NONE); }                        // (18 + 8: no payload, accepted)
  g_row = "header_block_past_the_end";
  CHECK(walk_one(bgzf_block(100, 1000, 1), 99) == FB_BLOCK);
  g_row = "header_isize_above_64_kib";
  CHECK(walk_one(bgzf_block(100, 0x10001, 1), 100) == FB_BLOCK);
}

// ---- slab layout
static void layout_row(const char* row, uint64_t nl, const uint64_t (&tot)[7], bool keep_bam4, size_t want_total) {
  g_row = row;
  const SlabLayout a = slab_layout(nl, tot, keep_bam4);
  const uint64_t nr = tot[0];
  // the pieces in their order, and what each has to hold: payload + one element of slack
  const size_t off[26] = {a.lrb, a.n_filt, a.n_seen, a.read_off, a.read_len, a.reads, a.quals, a.names, a.name_off, a.rq, a.is_reverse, a.mapq, a.hp, a.start_offset, a.end_offset, a.snp,
                          a.snp_off, a.meth, a.meth_off, a.has_meth, a.cig, a.cig_off, a.cig_ref_pos, a.bam4, a.bam4_off, a.total};
  const uint64_t need[25] = {(nl + 1) * 8, nl * 4, nl * 8, (nr + 1) * 8, (nr + 1) * 4, tot[1] + 1, tot[1] + 1, tot[2] + 1, (nr + 1) * 8, (nr + 1) * 8, nr + 1, nr + 1, (nr + 1) * 2, (nr + 1) * 4,
                             (nr + 1) * 4, (tot[3] + 1) * 4, (nr + 1) * 8, tot[4] + 1, (nr + 1) * 8, nr + 1, (tot[5] + 1) * 4, (nr + 1) * 8, (nr + 1) * 8, keep_bam4 ? tot[6] + 1 : 0,
                             keep_bam4 ? (nr + 1) * 8 : 0};
  CHECK(off[0] == 0);
  for (int i = 0; i < 25; ++i) { CHECK(off[i] % 64 == 0); CHECK(off[i] + need[i] <= off[i + 1]); CHECK(off[i + 1] - off[i] < need[i] + 64); }
  CHECK(a.total % 64 == 0 && a.total == want_total);
  if (!keep_bam4) CHECK(a.bam4 == a.bam4_off && a.bam4_off == a.total);
  // the two views of a slab: the same piece under the same name from either base, const or not
  struct DevView { uint64_t* read_off; uint32_t* read_len; uint8_t* reads; uint8_t* quals; char* names; uint64_t* name_off; double* rq; uint8_t* is_reverse; uint8_t* mapq; int16_t* hp;
                   int32_t* start_offset; int32_t* end_offset; int32_t* snp; uint64_t* snp_off; uint8_t* meth; uint64_t* meth_off; uint8_t* has_meth; uint32_t* cig; uint64_t* cig_off;
                   int64_t* cig_ref_pos; uint8_t* bam4; uint64_t* bam4_off; } d;
  HostOut v;
  std::vector<uint8_t> dev(a.total + 64), pin(a.total + 64);
  slab_view(d, dev.data(), a, keep_bam4); slab_view(v, pin.data(), a, keep_bam4);
  auto at = [](const void* p, const std::vector<uint8_t>& base) { return (size_t)((const uint8_t*)p - base.data()); };
  CHECK(at(d.read_off, dev) == a.read_off && at(v.read_off, pin) == a.read_off && at(d.read_len, dev) == a.read_len && at(v.read_len, pin) == a.read_len);
  CHECK(at(d.reads, dev) == a.reads && at(v.reads, pin) == a.reads && at(d.quals, dev) == a.quals && at(v.quals, pin) == a.quals && at(d.names, dev) == a.names && at(v.names, pin) == a.names);
  CHECK(at(d.name_off, dev) == a.name_off && at(v.name_off, pin) == a.name_off && at(d.rq, dev) == a.rq && at(v.rq, pin) == a.rq);
  CHECK(at(d.is_reverse, dev) == a.is_reverse && at(v.is_reverse, pin) == a.is_reverse && at(d.mapq, dev) == a.mapq && at(v.mapq, pin) == a.mapq && at(d.hp, dev) == a.hp && at(v.hp, pin) == a.hp);
  CHECK(at(d.start_offset, dev) == a.start_offset && at(v.start_offset, pin) == a.start_offset && at(d.end_offset, dev) == a.end_offset && at(v.end_offset, pin) == a.end_offset);
  CHECK(at(d.snp, dev) == a.snp && at(v.snp, pin) == a.snp && at(d.snp_off, dev) == a.snp_off && at(v.snp_off, pin) == a.snp_off);
  CHECK(at(d.meth, dev) == a.meth && at(v.meth, pin) == a.meth && at(d.meth_off, dev) == a.meth_off && at(v.meth_off, pin) == a.meth_off && at(d.has_meth, dev) == a.has_meth && at(v.has_meth, pin) == a.has_meth);
  CHECK(at(d.cig, dev) == a.cig && at(v.cig, pin) == a.cig && at(d.cig_off, dev) == a.cig_off && at(v.cig_off, pin) == a.cig_off && at(d.cig_ref_pos, dev) == a.cig_ref_pos && at(v.cig_ref_pos, pin) == a.cig_ref_pos);
  if (keep_bam4) CHECK(at(d.bam4, dev) == a.bam4 && at(v.bam4, pin) == a.bam4 && at(d.bam4_off, dev) == a.bam4_off && at(v.bam4_off, pin) == a.bam4_off);
  else CHECK(!d.bam4 && !d.bam4_off && !v.bam4 && !v.bam4_off);
  CHECK(!v.lrb && !v.n_filt && !v.n_seen && !v.dev_reads && v.n_reads == 0);  // (not the view's to set)
}
static void layouts() {
  const uint64_t none[7] = {0, 0, 0, 0, 0, 0, 0};
  layout_row("layout_empty", 0, none, false, 1344);           // lrb and the 20 per-read arrays: 64 bytes each
  layout_row("layout_empty_bam4", 0, none, true, 1472);       // ... and the two 4-bit pieces
  // 3 loci, 5 reads of 1000 bases, 70 name bytes, 7 mismatch offsets, 33 methylation values, 20 CIGAR operations, 502 bytes of 4-bit reads:
  // reads and quals 1024 each, names 128 (71), cig 128 (84), bam4 512 (503), the other twenty pieces 64
  const uint64_t small[7] = {5, 1000, 70, 7, 33, 20, 502};
  layout_row("layout_small_bam4", 3, small, true, 4096);
  layout_row("layout_small", 3, small, false, 3520);
  g_row = "layout_small_offsets";
  const SlabLayout a = slab_layout(3, small, true);
  CHECK(a.lrb == 0 && a.n_filt == 64 && a.n_seen == 128 && a.read_off == 192 && a.read_len == 256 && a.reads == 320 && a.quals == 1344 && a.names == 2368 && a.name_off == 2496);
  CHECK(a.rq == 2560 && a.is_reverse == 2624 && a.mapq == 2688 && a.hp == 2752 && a.start_offset == 2816 && a.end_offset == 2880 && a.snp == 2944 && a.snp_off == 3008);
  CHECK(a.meth == 3072 && a.meth_off == 3136 && a.has_meth == 3200 && a.cig == 3264 && a.cig_off == 3392 && a.cig_ref_pos == 3456 && a.bam4 == 3520 && a.bam4_off == 4032);
}

// ---- lease
struct CountingPool {
  int gives = 0; void* last = nullptr;
  void give(Slab& s) { ++gives; last = s.dev; s = Slab(); }
};
using Lease = SlabLeaseT<CountingPool>;
struct Holder { int before = 0; Lease lease; int after = 0; };
static void leases() {
  static char mem[4];
  auto slab = [](int k) { Slab s; s.dev = &mem[k]; s.pin = &mem[k]; s.cap = 64; s.device = 0; return s; };
  auto pool = std::make_shared<CountingPool>();
  g_row = "lease_dropped";
  { Lease l(slab(0), pool); CHECK(l.slab().dev == &mem[0] && l.slab().cap == 64 && pool->gives == 0); }
  CHECK(pool->gives == 1 && pool->last == &mem[0]);
  g_row = "lease_moved_then_dropped";
  pool->gives = 0;
  {
    Lease l(slab(1), pool);
    Lease m(std::move(l));
    CHECK(!l.slab().dev && !l.slab().pin && m.slab().dev == &mem[1] && pool->gives == 0);  // NOLINT (the moved-from lease is looked at on purpose)
    Lease n;
    n = std::move(m);
    CHECK(!m.slab().dev && n.slab().dev == &mem[1] && pool->gives == 0);  // NOLINT
  }
  CHECK(pool->gives == 1 && pool->last == &mem[1]);
  g_row = "lease_moved_into_a_holder";
  pool->gives = 0;
  {
    std::unique_ptr<Holder> h(new Holder());
    { Lease l(slab(2), pool); h->lease = std::move(l); }
    CHECK(pool->gives == 0 && h->lease.slab().dev == &mem[2]);
    h.reset();
    CHECK(pool->gives == 1 && pool->last == &mem[2]);
  }
  CHECK(pool->gives == 1);
  g_row = "lease_assigned_over";
  pool->gives = 0;
  {
    Lease l(slab(0), pool), m(slab(3), pool);
    l = std::move(m);   // the slab l held goes back now, m's when l is dropped
    CHECK(pool->gives == 1 && pool->last == &mem[0] && l.slab().dev == &mem[3]);
  }
  CHECK(pool->gives == 2 && pool->last == &mem[3]);
  g_row = "lease_empty";
  pool->gives = 0;
  { Lease l; Lease m(std::move(l)); Lease n(Slab(), pool); CHECK(!n.slab().dev); }
  CHECK(pool->gives == 0);
  // the pool lives as long as a lease does (a batch may be freed after its reader was closed)
  g_row = "lease_keeps_its_pool";
  std::weak_ptr<CountingPool> seen = pool;
  { Lease l(slab(1), pool); pool.reset(); CHECK(!seen.expired()); }
  CHECK(seen.expired());
}

int main() {
  windows();
  ranges();
  headers_and_chunks();
  refused_headers();
  layouts();
  leases();
  if (g_failed) { std::printf("ingest_plan_check: %d checks FAILED\n", g_failed); return 1; }
  std::printf("ingest_plan_check: all held\n");
  return 0;
}
