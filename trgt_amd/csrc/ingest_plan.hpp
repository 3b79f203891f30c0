// trgt_amd/csrc/ingest_plan.hpp -- everything the device-side read ingestion decides before it touches a file or the GPU, as pure functions
// of plain values: the windows of a locus, the compressed ranges of a call and where they go in the staging buffer, the BGZF block table
// read off the staged headers, the chunks' virtual offsets as positions in the inflated bytes, the layout of a batch's slab -- every
// fallback and every offset the kernels of ingest_dev.hip trust -- and the owner of a slab.  Standard library only (no HIP, no zlib, no file):
// tests/tools/ingest_plan_check.cpp holds it to literal values on the host compiler.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "inflate_dev.hpp"

namespace trgt {
namespace ingd {

// One fetch of extract_reads: the window of a locus and its chunks of the .bai as positions in the inflated bytes of the call
struct LocusDesc {
  int32_t tid, chunk_begin, chunk_end, pad;
  int64_t beg, end;                     // fetch window: region -+ flank_len
  int64_t region_start, region_end;     // locus.region
  int64_t clip_start, clip_end;         // clip_reads: region -+ 2 * flank_len
};
struct ChunkDesc { uint64_t lin0, lin1, lin_limit; };  // first record, end of the chunk, end of the inflated range the chunk lies in

// Why a call went back to the host path (RunOut::fallback)
enum : int { FB_NONE = 0, FB_BLOCK = 1 /* a block the device could not inflate or whose CRC-32 / ISIZE does not match */, FB_WALK = 2 /* a record the walk refuses */,
             FB_RESERVOIR = 3 /* (never set since the reservoir's random stream runs in walk_kernel; the value stays for the layout of the stats, and tests/test_ingest_device_gpu.py asserts that deep loci do not report it) */, FB_METH = 4 /* MM / ML beyond the kernel's LDS caps */ };

// The per-read arrays of a batch as one view: pieces of a slab's pinned mirror (64-byte aligned; dev_reads into the device copy), or the
// vectors of a batch the host path assembled
struct HostOut {
  int64_t n_reads = 0;
  uint64_t read_bytes = 0, name_bytes = 0, snp_n = 0, meth_n = 0, cig_n = 0, bam4_bytes = 0;
  const uint64_t* lrb = nullptr;            // [n_loci + 1]
  const int32_t* n_filt = nullptr; const int64_t* n_seen = nullptr;   // [n_loci]
  const uint64_t* read_off = nullptr; const uint32_t* read_len = nullptr; const uint8_t* reads = nullptr; const uint8_t* quals = nullptr;
  const char* names = nullptr; const uint64_t* name_off = nullptr;
  const double* rq = nullptr; const uint8_t* is_reverse = nullptr; const uint8_t* mapq = nullptr; const int16_t* hp = nullptr;
  const int32_t* start_offset = nullptr; const int32_t* end_offset = nullptr;
  const int32_t* snp = nullptr; const uint64_t* snp_off = nullptr;
  const uint8_t* meth = nullptr; const uint64_t* meth_off = nullptr; const uint8_t* has_meth = nullptr;
  const uint32_t* cig = nullptr; const uint64_t* cig_off = nullptr; const int64_t* cig_ref_pos = nullptr;
  const uint8_t* bam4 = nullptr; const uint64_t* bam4_off = nullptr;
  const uint8_t* dev_reads = nullptr;       // the ASCII read blob in HBM (same offsets as `reads`)
};

using VoffPair = std::pair<uint64_t, uint64_t>;  // a chunk of the .bai: two virtual offsets (compressed offset << 16 | offset in the block)

inline uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---------------------------------------------------------------------------------------------- the windows of a locus
// (the fetch window starts at 0 at the earliest, like the host path's; clip_reads cuts where it cuts.  The chunks are the caller's.)
inline LocusDesc locus_windows(int32_t tid, int64_t start, int64_t end, int64_t flank_len) {
  LocusDesc d;
  d.tid = tid; d.chunk_begin = 0; d.chunk_end = 0; d.pad = 0;
  d.beg = std::max<int64_t>(0, start - flank_len); d.end = end + flank_len;
  d.region_start = start; d.region_end = end;
  d.clip_start = start - 2ll * flank_len; d.clip_end = end + 2ll * flank_len;
  return d;
}

// The chunks of every locus, one locus after the other (chunk_begin / chunk_end say whose): query(tid, beg, end) is the .bai.  A locus on a
// contig the BAM does not have (tid < 0) gets none -- "Fetch error" is a warning in the reference, the locus has no reads.
template <class Query>
inline std::vector<VoffPair> locus_chunks(std::vector<LocusDesc>& loci, Query&& query) {
  std::vector<VoffPair> cv;
  for (LocusDesc& d : loci) {
    d.chunk_begin = (int32_t)cv.size();
    if (d.tid >= 0) for (auto& ch : query(d.tid, d.beg, d.end)) cv.push_back(ch);
    d.chunk_end = (int32_t)cv.size();
  }
  return cv;
}

// ---------------------------------------------------------------------------------------------- compressed ranges
// The chunks of a call as ranges [first, second] of compressed offsets (where their first and last blocks start), merged where less than a
// block apart; a range is read up to `read_end` (its last block whole, and the 64 bytes the kernels may read beyond) and staged at `src_at`.
struct ReadPiece { uint64_t file_off, src_off; size_t n; };  // file bytes [file_off, + n) -> staging buffer at src_off
struct RangePlan {
  uint64_t fsize = 0;
  std::vector<VoffPair> ranges;
  std::vector<uint64_t> read_end, src_at;
  uint64_t src_total = 0;
  std::vector<ReadPiece> pieces;            // at most 4 MiB each: what one reader thread takes at a time
};
inline RangePlan plan_ranges(const std::vector<VoffPair>& chunks, uint64_t fsize) {
  RangePlan rp;
  rp.fsize = fsize;
  std::vector<VoffPair> all;
  for (auto& c : chunks) all.emplace_back(c.first >> 16, c.second >> 16);
  std::sort(all.begin(), all.end());
  for (auto& r : all) {
    if (!rp.ranges.empty() && r.first <= rp.ranges.back().second + 0x10000) rp.ranges.back().second = std::max(rp.ranges.back().second, r.second);
    else rp.ranges.push_back(r);
  }
  rp.read_end.resize(rp.ranges.size()); rp.src_at.resize(rp.ranges.size());
  for (size_t i = 0; i < rp.ranges.size(); ++i) {
    const uint64_t c0 = rp.ranges[i].first, c1 = std::min<uint64_t>(fsize, rp.ranges[i].second + 0x10000 + 64);
    rp.read_end[i] = c1; rp.src_at[i] = rp.src_total;
    if (c1 > c0) rp.src_total += ((c1 - c0) + 63) & ~63ull;
    for (uint64_t o = c0; o < c1; o += 4u << 20) rp.pieces.push_back({o, rp.src_at[i] + (o - c0), (size_t)std::min<uint64_t>(c1 - o, 4u << 20)});
  }
  return rp;
}

// ---------------------------------------------------------------------------------------------- the block table
// The BGZF headers and footers of the staged ranges: payloads, where they inflate to (the blocks of a range end to end, so a record may run
// across blocks as in the file), the footers' CRC-32.  `known`: every block met, also the empty ones (which are not inflated), by `coff`.
struct KnownBlock { uint64_t coff, lin; uint32_t isize, range; };
struct BlockWalk {
  int fallback = FB_NONE;                   // FB_BLOCK: a header the walk does not take (the host path then says what is wrong)
  std::vector<infl::BlockDesc> blocks; std::vector<uint32_t> crcs;
  std::vector<KnownBlock> known;
  std::vector<uint64_t> lin_end;            // per range: where its inflated bytes end
  uint64_t infl_bytes = 0;
};
inline BlockWalk walk_block_headers(const uint8_t* src, uint64_t src_bytes, const RangePlan& rp) {
  BlockWalk w;
  auto fall = [&]() { w = BlockWalk(); w.fallback = FB_BLOCK; return w; };
  if (src_bytes < rp.src_total) return fall();
  w.lin_end.resize(rp.ranges.size());
  uint64_t lin = 0;
  for (size_t i = 0; i < rp.ranges.size(); ++i) {
    const uint64_t c0 = rp.ranges[i].first, cend = rp.read_end[i];
    uint64_t coff = c0;
    while (coff <= rp.ranges[i].second && coff < rp.fsize) {
      if (coff + 18 > cend) return fall();
      const uint8_t* hp = src + rp.src_at[i] + (coff - c0);
      if (hp[0] != 31 || hp[1] != 139 || hp[2] != 8 || !(hp[3] & 4)) return fall();
      const uint32_t xlen = hp[10] | (hp[11] << 8);
      if (coff + 12 + xlen > cend) return fall();
      uint32_t bsize = 0; bool found = false;
      for (uint32_t k = 0; k + 4 <= xlen;) {
        const uint32_t slen = hp[12 + k + 2] | (hp[12 + k + 3] << 8);
        if (hp[12 + k] == 'B' && hp[12 + k + 1] == 'C' && slen == 2 && k + 6 <= xlen) { bsize = hp[12 + k + 4] | (hp[12 + k + 5] << 8); found = true; break; }
        k += 4 + slen;
      }
      if (!found) return fall();
      const uint32_t total = bsize + 1, hdr = 12 + xlen;
      if (total < hdr + 8 || coff + total > cend) return fall();
      const uint32_t isize = le32(hp + total - 4);
      if (isize > 0x10000) return fall();
      w.known.push_back(KnownBlock{coff, lin, isize, (uint32_t)i});
      if (isize) {
        w.blocks.push_back(infl::BlockDesc{rp.src_at[i] + (coff - c0) + hdr, lin, total - hdr - 8, isize});
        w.crcs.push_back(le32(hp + total - 8));
        lin += isize;
      }
      coff += total;
    }
    w.lin_end[i] = lin;
    lin = ((lin + 63) & ~63ull) + 64;  // (a gap between the ranges: nothing of one is read as the other's)
  }
  w.infl_bytes = lin;
  return w;
}

// ---------------------------------------------------------------------------------------------- the chunks as positions in the inflated bytes
// FB_NONE, or FB_WALK for a chunk that starts in a block the walk did not meet or behind that block's end
inline int place_chunks(const std::vector<VoffPair>& chunks, const BlockWalk& w, std::vector<ChunkDesc>& cd) {
  cd.assign(chunks.size(), ChunkDesc{0, 0, 0});
  auto find = [&](uint64_t coff) -> const KnownBlock* {
    auto it = std::lower_bound(w.known.begin(), w.known.end(), coff, [](const KnownBlock& k, uint64_t c) { return k.coff < c; });
    return it != w.known.end() && it->coff == coff ? &*it : nullptr;
  };
  for (size_t c = 0; c < chunks.size(); ++c) {
    const KnownBlock* a = find(chunks[c].first >> 16);
    if (!a || (chunks[c].first & 0xFFFF) > a->isize) return FB_WALK;
    const KnownBlock* b = find(chunks[c].second >> 16);
    cd[c].lin0 = a->lin + (chunks[c].first & 0xFFFF);
    cd[c].lin_limit = w.lin_end[a->range];
    cd[c].lin1 = b && b->range == a->range ? std::min<uint64_t>(b->lin + std::min<uint64_t>(chunks[c].second & 0xFFFF, b->isize), cd[c].lin_limit) : cd[c].lin_limit;
  }
  return FB_NONE;
}

// ---------------------------------------------------------------------------------------------- the slab of a batch
// Every array a 64-byte aligned piece with one element of slack, in this order; `total` bytes in all (the pool adds 64).  tot[]: reads, read
// bytes, name bytes, mismatch offsets, methylation values, CIGAR operations, 4-bit read bytes (read_sizes_kernel's Counters::tot).
struct SlabLayout {
  size_t lrb, n_filt, n_seen, read_off, read_len, reads, quals, names, name_off, rq, is_reverse, mapq, hp, start_offset, end_offset, snp, snp_off, meth, meth_off, has_meth, cig,
         cig_off, cig_ref_pos, bam4, bam4_off, total;
};
inline SlabLayout slab_layout(uint64_t n_loci, const uint64_t tot[7], bool keep_bam4) {
  const uint64_t nl = n_loci, nr = tot[0], n_bytes = tot[1], n_name = tot[2], n_snp = tot[3], n_meth = tot[4], n_cig = tot[5], n_bam4 = keep_bam4 ? tot[6] : 0;
  size_t at = 0;
  auto piece = [&](size_t bytes) { const size_t a = at; at += (bytes + 63) & ~(size_t)63; return a; };
  SlabLayout a;
  a.lrb = piece(((size_t)nl + 1) * 8); a.n_filt = piece((size_t)nl * 4); a.n_seen = piece((size_t)nl * 8); a.read_off = piece((nr + 1) * 8); a.read_len = piece((nr + 1) * 4);
  a.reads = piece(n_bytes + 1); a.quals = piece(n_bytes + 1); a.names = piece(n_name + 1); a.name_off = piece((nr + 1) * 8); a.rq = piece((nr + 1) * 8);
  a.is_reverse = piece(nr + 1); a.mapq = piece(nr + 1); a.hp = piece((nr + 1) * 2); a.start_offset = piece((nr + 1) * 4); a.end_offset = piece((nr + 1) * 4);
  a.snp = piece((n_snp + 1) * 4); a.snp_off = piece((nr + 1) * 8); a.meth = piece(n_meth + 1); a.meth_off = piece((nr + 1) * 8); a.has_meth = piece(nr + 1);
  a.cig = piece((n_cig + 1) * 4); a.cig_off = piece((nr + 1) * 8); a.cig_ref_pos = piece((nr + 1) * 8);
  a.bam4 = piece(keep_bam4 ? n_bam4 + 1 : 0); a.bam4_off = piece(keep_bam4 ? (nr + 1) * 8 : 0);
  a.total = at;
  return a;
}
// The one list of which piece is which per-read array: View is the kernels' OutPtrs over the device copy, or HostOut over the pinned mirror
template <class View>
inline void slab_view(View& v, uint8_t* base, const SlabLayout& a, bool keep_bam4) {
  auto set = [&](auto& p, size_t off) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off); };
  set(v.read_off, a.read_off); set(v.read_len, a.read_len); set(v.reads, a.reads); set(v.quals, a.quals); set(v.names, a.names); set(v.name_off, a.name_off);
  set(v.rq, a.rq); set(v.is_reverse, a.is_reverse); set(v.mapq, a.mapq); set(v.hp, a.hp); set(v.start_offset, a.start_offset); set(v.end_offset, a.end_offset);
  set(v.snp, a.snp); set(v.snp_off, a.snp_off); set(v.meth, a.meth); set(v.meth_off, a.meth_off); set(v.has_meth, a.has_meth);
  set(v.cig, a.cig); set(v.cig_off, a.cig_off); set(v.cig_ref_pos, a.cig_ref_pos);
  v.bam4 = nullptr; v.bam4_off = nullptr;
  if (keep_bam4) { set(v.bam4, a.bam4); set(v.bam4_off, a.bam4_off); }
}

// ---------------------------------------------------------------------------------------------- who holds a slab
// A device slab + its pinned mirror: the per-read arrays of one batch.  They move into the batch (the read bytes stay in HBM for
// trgt_locus_batch) and come back to the pool when the batch is freed.
struct Slab { void* dev = nullptr; void* pin = nullptr; size_t cap = 0; int device = -1; };
// Move-only owner of a slab and the pool it returns to (Pool: SlabPool of ingest_dev.hpp; anything with give(Slab&)): whoever drops the
// lease -- a failed call, an exception, the batch when it is freed -- gives the slab back, once.
template <class Pool>
class SlabLeaseT {
 public:
  SlabLeaseT() = default;
  SlabLeaseT(const Slab& s, std::shared_ptr<Pool> pool) : slab_(s), pool_(std::move(pool)) {}
  SlabLeaseT(SlabLeaseT&& o) noexcept : slab_(o.slab_), pool_(std::move(o.pool_)) { o.slab_ = Slab(); }
  SlabLeaseT& operator=(SlabLeaseT&& o) noexcept {
    if (this != &o) { give_back(); slab_ = o.slab_; pool_ = std::move(o.pool_); o.slab_ = Slab(); }
    return *this;
  }
  SlabLeaseT(const SlabLeaseT&) = delete;
  SlabLeaseT& operator=(const SlabLeaseT&) = delete;
  ~SlabLeaseT() { give_back(); }
  const Slab& slab() const { return slab_; }

 private:
  void give_back() { if (pool_ && (slab_.dev || slab_.pin)) pool_->give(slab_); pool_.reset(); slab_ = Slab(); }
  Slab slab_;
  std::shared_ptr<Pool> pool_;
};

}  // namespace ingd
}  // namespace trgt
