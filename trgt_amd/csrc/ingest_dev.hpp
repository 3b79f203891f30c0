// trgt_amd/csrc/ingest_dev.hpp -- host interface of the device-side read ingestion (ingest_dev.hip): everything of extract_reads /
// HiFiRead::from_hts_rec / clip_reads (src/trgt/workflows/tr.rs:268-361, 186-196; reads/read.rs:55-141; reads/snp.rs:51-79;
// reads/clip_region.rs:19-184) that touches inflated BAM bytes, as kernels behind the device inflate, so that those bytes never leave HBM.
#pragma once
#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "inflate_dev.hpp"
#include "ingest_plan.hpp"

struct trgt_ingest_batch;

namespace trgt {
// ingest.hip: the slab of a device-ingested batch (false: the batch has none)
bool ingest_batch_slab(const trgt_ingest_batch* b, const void** dev, const void** pin, size_t* bytes, int* device);

namespace ingd {

// the one clock of both files: milliseconds, steady
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// (the slabs of the device a call runs on; `give` has no HIP call: a lease may outlive every stream)
struct SlabPool {
  std::mutex mu;
  std::vector<Slab> idle;
  ~SlabPool();
  bool take(int device, size_t bytes, Slab& out);
  void give(Slab& s);
};
using SlabLease = SlabLeaseT<SlabPool>;

struct RunIn {
  uint64_t src_bytes = 0;                   // compressed bytes staged in slot_src()
  int64_t n_blocks = 0; const infl::BlockDesc* blocks = nullptr; const uint32_t* crc = nullptr;  // BGZF blocks: payload -> inflated position; CRC-32 of the footer
  uint64_t infl_bytes = 0;
  int64_t n_loci = 0; const LocusDesc* loci = nullptr;
  int64_t n_chunks = 0; const ChunkDesc* chunks = nullptr;
  uint32_t reservoir = 750; double min_rq = 0.98; bool keep_bam4 = false; int waves_per_cu = 0;
};
// (the lease: whoever drops a RunOut whose slab was taken -- an error leg, an exception -- returns the slab to its pool)
struct RunOut { int fallback = FB_NONE; SlabLease lease; HostOut out; double ms_upload = 0, ms_inflate = 0, ms_walk = 0, ms_reads = 0, ms_download = 0; uint64_t blocks_host_inflated = 0; };

class Slot;
Slot* slot_create(int device, std::string& err);
void slot_destroy(Slot* s);
uint8_t* slot_src(Slot* s, size_t bytes, std::string& err);   // pinned staging for the compressed bytes of a call (valid until the next call)
// 0 ok (out.fallback says whether the results are usable), < 0 TRGT_ERR_*
int slot_run(Slot* s, const RunIn& in, const std::shared_ptr<SlabPool>& pool, RunOut& out, std::string& err);


// crc32_blocks_kernel for another stage's blocks (the writer's BGZF blocks, bam_records_dev.hip): d_out[b] = CRC-32 of d_data[dst_off .. + dst_len)
// of block b (src_off / src_len unused; 3 bytes of slack behind the data).  d_tab: crc32_tables_bytes() device bytes, a copy of crc32_tables_make's.
size_t crc32_tables_bytes();
void crc32_tables_make(void* host);
void crc32_blocks_launch(void* hip_stream, const uint8_t* d_data, const infl::BlockDesc* d_blocks, uint32_t n, const void* d_tab, uint32_t* d_out);

#ifdef TRGT_DEV_BUILD
// developer build only (trgt_dev_rng_draws, ingest.hip): `count` draws of walk_kernel's DevRng by one wave of GPU `device` -- n[k] == 0: raw
// next_u32, else range(n[k]) with n[k] < 2^32; key == nullptr: expanded from `seed`
int dev_rng_draws(int device, uint64_t seed, const uint32_t* key, uint64_t counter, int rounds, int64_t count, const uint64_t* n, uint64_t* out, std::string& err);
#endif

}  // namespace ingd
}  // namespace trgt
