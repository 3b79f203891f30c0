// trgt_amd/csrc/bam_records_dev.hpp -- host interface of the device-side assembly of the spanning-BAM records (bam_records_dev.hip):
// BamWriter::write (src/trgt/writers/write_bam.rs:72-144) with HiFiRead::clip_bases (src/trgt/reads/clip_bases.rs:9-120) as kernels over the
// per-read arrays the device ingestion left in HBM, so that the record bytes of a batch are born where they are deflated.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

struct trgt_hip_ctx;

namespace trgt {
namespace brec {

// The per-read arrays of a device-ingested batch, as DEVICE addresses (the slab of ingest_dev.hip: same layout as the pinned mirror)
struct BatchDev {
  int64_t n_reads = 0;
  const uint64_t* read_off = nullptr; const uint32_t* read_len = nullptr; const uint8_t* reads = nullptr; const uint8_t* quals = nullptr;
  const char* names = nullptr; const uint64_t* name_off = nullptr; const double* rq = nullptr; const uint8_t* is_reverse = nullptr; const uint8_t* mapq = nullptr;
  const int16_t* hp = nullptr; const int32_t* start_offset = nullptr; const int32_t* end_offset = nullptr; const int32_t* snp = nullptr; const uint64_t* snp_off = nullptr;
  const uint8_t* meth = nullptr; const uint64_t* meth_off = nullptr; const uint8_t* has_meth = nullptr; const uint32_t* cig = nullptr; const uint64_t* cig_off = nullptr;
  const int64_t* cig_ref_pos = nullptr;
};
// One kept read in record order (loci in batch order, within a locus by read_rank) with its results: 20 bytes per read go up
struct RecIn { uint32_t read, locus; int32_t span_start, span_end, classification; };
struct LocusIn { int32_t tid; uint32_t id_off, id_len; };   // the contig in the BAM header, the locus id (TR:Z) in the id blob

// Why the kernels refused a batch (it is then formatted by the host path, which reports what it reports)
enum : uint32_t { FLAG_CIGAR_SHORT = 1, FLAG_CIGAR_OPS = 2, FLAG_RANGE = 4 /* a result or an index outside the read's own arrays */ };

struct Assembled {
  uint32_t flags = 0;          // FLAG_*: nothing was written when != 0
  uint64_t n_records = 0;      // records written (kept reads minus the ones the skip rules drop)
  uint64_t rec_bytes = 0;      // their bytes
  uint64_t stream_bytes = 0;   // carried tail + records: what lies in the engine's stream buffer
  uint64_t h2d_bytes = 0;
};
// What finish() hands back: the full 0xFF00-byte blocks of the stream, then its tail.  The pointers are pinned memory of the engine, valid
// until its next call.
struct Finished {
  uint64_t n_blocks = 0;
  bool deflated = false;                 // the blocks went through the device deflate
  // deflated: block k's payload at payload + k * 0x10000, len[k] bytes, crc[k] its CRC-32; a block with len 0 (or too long for a BGZF block)
  // was declined: its 0xFF00 bytes are at raw + raw_at[k]; tail: the bytes behind the last full block
  const uint8_t* payload = nullptr; const uint32_t* len = nullptr; const uint32_t* crc = nullptr; const uint64_t* raw_at = nullptr;
  const uint8_t* tail = nullptr; uint64_t tail_bytes = 0;
  // not deflated: raw is the whole stream (blocks + tail), for zlib
  const uint8_t* raw = nullptr; uint64_t raw_bytes = 0;
  uint64_t d2h_bytes = 0;
};

class Engine;
Engine* engine_create(int device, std::string& err, int* n_devices);
void engine_destroy(Engine* e);
// sizes, offsets, fill: the records of the batch behind `tail` in the engine's stream buffer.  Synchronous: nothing of the arguments is
// referenced when it returns.
int assemble(Engine* e, const BatchDev& b, const RecIn* recs, size_t n_recs, const LocusIn* loci, size_t n_loci, const char* id_blob, size_t id_bytes,
             uint32_t flank, bool keep_unmapped, const uint8_t* tail, size_t tail_len, Assembled& out, std::string& err);
// CRC-32 + deflate (defl != nullptr and at least `min_dev_blocks` full blocks) + what must come back.  Synchronous.
int finish(Engine* e, trgt_hip_ctx* defl, uint64_t min_dev_blocks, Finished& out, std::string& err);

}  // namespace brec
}  // namespace trgt
