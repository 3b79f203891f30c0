// trgt_amd/csrc/writers.hip -- the step behind the GPU path, host C++ (no device code):
//   VcfWriter::new                                        src/trgt/writers/write_vcf.rs:19-92
//   BamWriter::create_header                              src/trgt/writers/write_bam.rs:33-65
// and the files themselves: BgzfOut, the write call as the stages of a WriteCall (check_args, format_all, map_device_batch, plan_records,
// assemble_on_device, hand_over with flush_pieces / flush_device), write-behind.  What a locus looks like -- the VCF line, set_gt, the AM
// field, the spanning-BAM record, clip_bases -- is writer_format.hpp (no HIP, held by tests/tools/writer_format_check.cpp).
// Input: a batch of the native ingestion (trgt_ingest_batch: catalog fields, clipped reads with their HiFiRead fields) and the result
// arrays trgt_locus_batch filled for it.  The reference writes through htslib; here VCF lines are formatted directly (BGZF-compressed when
// the path ends in .gz -- the reference's bcf::Writer compresses) and BAM records are encoded and BGZF-compressed with zlib.
// trgt_writer_set_records_device: the records of a device-ingested batch are assembled by bam_records_dev.hip's kernels instead (same bytes).
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "bam_records_dev.hpp"
#include "bgzf_block.hpp"
#include "crc32_fast.hpp"
#include "ingest_dev.hpp"
#include "writer_format.hpp"
#include "../../include/trgt_hip.h"

extern "C" {
const char* trgt_ingest_header_text(const trgt_ingest* h);
int32_t trgt_ingest_n_contigs(const trgt_ingest* h);
const char* trgt_ingest_contig_name(const trgt_ingest* h, int32_t i);
uint32_t trgt_ingest_contig_length(const trgt_ingest* h, int32_t i);
}

namespace {

struct BgzfOut {  // a file, plain or as a series of BGZF blocks (cut every 0xFF00 bytes of payload, whatever the number of threads)
  FILE* f = nullptr; bool bgzf = false; std::vector<uint8_t> buf; int threads = 1; int level = 6;
  bool open(const char* path, bool compress) { f = std::fopen(path, "wb"); bgzf = compress; return f != nullptr; }
  static bool deflate_block(const uint8_t* d, size_t n, std::vector<uint8_t>& out, int level = 6) {
    out.resize(0x10000 + 64);
    z_stream zs; std::memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t*>(d); zs.avail_in = (uInt)n; zs.next_out = out.data() + 18; zs.avail_out = (uInt)out.size() - 18 - 8;
    const int rc = deflate(&zs, Z_FINISH);
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) return false;
    frame(out, zs.total_out, n ? trgt::crc32_fast(d, n) : 0u, n);
    return true;
  }
  bool block(const uint8_t* d, size_t n) { std::vector<uint8_t> out; return deflate_block(d, n, out, level) && std::fwrite(out.data(), 1, out.size(), f) == out.size(); }
  // the BGZF framing of a block whose clen bytes of payload lie at out[18..]: header in front, CRC-32 and size of its n bytes of data behind
  static void frame(std::vector<uint8_t>& out, size_t clen, uint32_t crc, size_t n) {
    const size_t total = 18 + clen + 8;
    out.resize(total);
    static const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
    std::memcpy(out.data(), head, 16);
    out[16] = (uint8_t)((total - 1) & 0xFF); out[17] = (uint8_t)((total - 1) >> 8);
    for (int i = 0; i < 4; ++i) { out[18 + clen + i] = (uint8_t)(crc >> (8 * i)); out[22 + clen + i] = (uint8_t)((uint32_t)n >> (8 * i)); }
  }
  // a BGZF block around a payload that is deflated already (trgt_deflate_blocks)
  static void frame_block(const uint8_t* d, size_t n, const uint8_t* payload, size_t clen, std::vector<uint8_t>& out) { frame_block(n ? trgt::crc32_fast(d, n) : 0u, n, payload, clen, out); }
  static void frame_block(uint32_t crc, size_t n, const uint8_t* payload, size_t clen, std::vector<uint8_t>& out) {
    out.resize(18 + clen + 8);
    std::memcpy(out.data() + 18, payload, clen);
    frame(out, clen, crc, n);
  }
  trgt_hip_ctx* dev = nullptr;   // trgt_writer_params.deflate_device: the full blocks of a flush are deflated on this context's GPU
  std::string dev_err;           // a device deflate that FAILED fails the write (no silent host-only run, like ingest_device); this says why
  std::atomic<int64_t> n_dev{0}, n_declined{0}, n_host{0};  // (read by trgt_writer_device_stats while the write-behind thread may run) blocks the device deflated / declined (zlib took them) / zlib deflated because the flush was too small or no device was named
  std::atomic<int64_t> link_up{0}, link_down{0};  // bytes the BAM's blocks moved to / from the device so far (TRGT_WRITER_TRACE)
  std::vector<uint8_t> dev_out; std::vector<uint64_t> dev_soff, dev_doff; std::vector<uint32_t> dev_slen, dev_cap, dev_len;
  // the full blocks of buf: deflated by `threads` workers (a block is independent of its neighbours) -- or on the GPU in one go, the
  // workers then only frame them (CRC-32) and deflate what the device declined -- written in order
  bool flush_full_blocks() {
    const size_t nb = buf.size() / 0xFF00;
    if (!nb) return true;
    std::vector<std::vector<uint8_t>> outs(nb);
    std::atomic<size_t> next{0}; std::atomic<int> failed{0};
    constexpr size_t DEV_SLOT = 0x10000, DEV_CAP = 0xFF00;  // room per block on the device side: payload + 26 must fit a BGZF block; 256 bytes of slack between the regions
    bool on_dev = false;
    if (dev && nb >= 16) {  // (a handful of blocks is not worth the round trip)
      dev_out.resize(nb * DEV_SLOT + 64); dev_soff.resize(nb); dev_doff.resize(nb); dev_slen.assign(nb, 0xFF00u); dev_cap.assign(nb, (uint32_t)DEV_CAP); dev_len.assign(nb, 0u);
      for (size_t k = 0; k < nb; ++k) { dev_soff[k] = k * 0xFF00; dev_doff[k] = k * DEV_SLOT; }
      const int rc = trgt_deflate_blocks(dev, (int64_t)nb, buf.data(), dev_soff.data(), dev_slen.data(), dev_out.data(), dev_doff.data(), dev_cap.data(), dev_len.data());
      if (rc != TRGT_OK) { dev_err = std::string("deflate_device: ") + trgt_hip_last_error(dev); return false; }
      on_dev = true;
      uint32_t widest = 0;
      for (size_t k = 0; k < nb; ++k) { if (trgt::bgzf_payload_fits(dev_len[k])) ++n_dev; else ++n_declined; widest = std::max(widest, dev_len[k]); }
      link_up += (int64_t)(nb * 0xFF00 + nb * 24); link_down += (int64_t)(nb * 4 + nb * (((size_t)widest + 3) & ~(size_t)3));
    } else n_host += (int64_t)nb;
    auto work = [&]() {
      try {
        for (;;) {
          const size_t k = next.fetch_add(1);
          if (k >= nb) break;
          if (on_dev && trgt::bgzf_payload_fits(dev_len[k])) frame_block(buf.data() + k * 0xFF00, 0xFF00, dev_out.data() + dev_doff[k], dev_len[k], outs[k]);
          else if (!deflate_block(buf.data() + k * 0xFF00, 0xFF00, outs[k], level)) failed = 1;
        }
      } catch (const std::exception&) { failed = 1; }
    };
    const int nt = (int)std::min<size_t>((size_t)std::max(1, threads), nb);
    if (nt <= 1) work();
    else { std::vector<std::thread> th; for (int t = 0; t < nt; ++t) th.emplace_back(work); for (auto& t : th) t.join(); }
    if (failed) return false;
    for (auto& o : outs) if (std::fwrite(o.data(), 1, o.size(), f) != o.size()) return false;
    buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)(nb * 0xFF00));
    return true;
  }
  // append() + one flush() per batch: the flush then sees all the blocks of the batch at once (enough for the workers, or for the device)
  bool append(const void* d, size_t n) {
    if (!bgzf) return std::fwrite(d, 1, n, f) == n;
    const uint8_t* p = (const uint8_t*)d;
    buf.insert(buf.end(), p, p + n);
    return true;
  }
  bool flush() { return !bgzf || flush_full_blocks(); }
  bool write(const void* d, size_t n) { return append(d, n) && flush(); }
  bool close() {
    bool ok = true;
    if (f) {
      if (bgzf) {  // what is left: full blocks first (an append without its flush, after an error), then the short one, + the empty EOF block
        ok = flush_full_blocks();
        if (!buf.empty()) ok = block(buf.data(), buf.size()) && ok;
        buf.clear(); ok = block(nullptr, 0) && ok;
      }
      ok = std::fclose(f) == 0 && ok; f = nullptr;
    }
    return ok;
  }
};

namespace br = trgt::brec;
namespace wf = trgt::wfmt;
using wf::put32;

inline bool ends_with(const std::string& s, const char* suf) { const size_t n = std::strlen(suf); return s.size() >= n && s.compare(s.size() - n, n, suf) == 0; }

}  // namespace

struct trgt_writer {
  std::string err, sample;
  BgzfOut vcf, bam;
  bool has_bam = false, keep_unmapped = false;
  int32_t flank_len = 50;
  int threads = 1;
  std::vector<std::string> contigs;
  trgt_hip_ctx* dev = nullptr;  // owned: the context of trgt_writer_params.deflate_device
  // write_behind (ABI 11): the formatted pieces of a batch are appended, deflated and written by a thread of the writer's own while the
  // caller formats the next batch; one batch in flight; what that thread reports is returned by the next write or by the close
  bool write_behind = false;
  std::thread bg; int bg_rc = TRGT_OK; std::string bg_err;
  // trgt_writer_set_records_device: the records of the batches that carry device arrays on GPU rec_device are assembled there
  trgt::brec::Engine* rec = nullptr; int32_t rec_device = -1, dev_ordinal = -1;
  std::atomic<int64_t> rec_stats[5] = {{0}, {0}, {0}, {0}, {0}};
  bool wrote = false;
  int bg_wait() { if (bg.joinable()) bg.join(); if (bg_rc != TRGT_OK && !bg_err.empty()) { err = bg_err; bg_err.clear(); } const int rc = bg_rc; bg_rc = TRGT_OK; return rc; }
  ~trgt_writer() { if (bg.joinable()) bg.join(); if (rec) trgt::brec::engine_destroy(rec); if (dev) trgt_hip_destroy(dev); }
};

namespace {

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What the "[writer]" line of TRGT_WRITER_TRACE says about one batch (phase times on stderr; tools/writer_records_ab.py parses it)
struct Trace {
  bool on = false, device = false;      // device: the records were assembled there, between t_dev and t_fmt
  double t0 = 0, t_dev = 0, t_fmt = 0;  // the formatting starts / the assembly starts / both are done, the flush starts
  int64_t nl = 0; int nt = 1; size_t vcf_bytes = 0; uint64_t rec_bytes = 0, n_records = 0;
};
void trace_line(const Trace& t, const BgzfOut& bo) {
  char what[192];
  if (t.device) std::snprintf(what, sizeof what, "%zu B of VCF; %llu B of BAM records in %llu records on the device: %.1f ms of it", t.vcf_bytes, (unsigned long long)t.rec_bytes, (unsigned long long)t.n_records, t.t_fmt - t.t_dev);
  else std::snprintf(what, sizeof what, "%zu B of VCF, %llu B of BAM records", t.vcf_bytes, (unsigned long long)t.rec_bytes);
  std::fprintf(stderr, "[writer] %lld loci, %d threads: formatting %.1f ms (%s), deflate + write %.1f ms, link %lld B up / %lld B down so far\n", (long long)t.nl, t.nt, t.t_fmt - t.t0, what,
               now_ms() - t.t_fmt, (long long)bo.link_up.load(), (long long)bo.link_down.load());
}

// The formatted batch: one piece per worker, in locus order.  Owned by the call, or by the write-behind thread once it is handed over:
// a flush references nothing of the batch or of the results.
struct Pieces { std::vector<std::string> lines, errs; std::vector<std::vector<uint8_t>> recs; Trace tr; };
using Flush = int (*)(trgt_writer*, Pieces&, std::string&);

// Host records: what precedes the first failing locus is written, as a serial writer would have; msg: what went wrong
int flush_pieces(trgt_writer* w, Pieces& p, std::string& msg) {
  for (size_t t = 0; t < p.lines.size(); ++t) {
    if (!p.lines[t].empty() && !w->vcf.append(p.lines[t].data(), p.lines[t].size())) { msg = "cannot write the VCF"; return TRGT_ERR_INVALID; }
    if (!p.recs[t].empty() && !w->bam.append(p.recs[t].data(), p.recs[t].size())) { msg = "cannot write the BAM"; return TRGT_ERR_INVALID; }
    if (!p.errs[t].empty()) { w->vcf.flush(); w->bam.flush(); msg = p.errs[t]; return TRGT_ERR_INVALID; }
  }
  if (!w->vcf.flush()) { msg = "cannot write the VCF"; return TRGT_ERR_INVALID; }
  if (!w->bam.flush()) { msg = w->bam.dev_err.empty() ? "cannot write the BAM" : w->bam.dev_err; return TRGT_ERR_INVALID; }
  return TRGT_OK;
}
// Device records: the VCF lines, then the stream the engine holds -- CRC-32, deflate, what comes back, the files
int flush_device(trgt_writer* w, Pieces& p, std::string& msg) {
  for (auto& s : p.lines) if (!s.empty() && !w->vcf.append(s.data(), s.size())) { msg = "cannot write the VCF"; return TRGT_ERR_INVALID; }
  if (!w->vcf.flush()) { msg = "cannot write the VCF"; return TRGT_ERR_INVALID; }
  BgzfOut& bo = w->bam;
  br::Finished Fi;
  if (const int frc = br::finish(w->rec, bo.dev, 16, Fi, msg)) return frc;
  bo.link_down += (int64_t)Fi.d2h_bytes;
  if (!Fi.deflated) {  // zlib: the stream is the buffer (what it held is the stream's head)
    bo.buf.assign(Fi.raw, Fi.raw + Fi.raw_bytes);
    if (!bo.flush()) { msg = bo.dev_err.empty() ? "cannot write the BAM" : bo.dev_err; return TRGT_ERR_INVALID; }
    return TRGT_OK;
  }
  bo.link_up += (int64_t)(Fi.n_blocks * 24);
  std::vector<uint8_t> out;
  for (uint64_t k = 0; k < Fi.n_blocks; ++k) {
    if (trgt::bgzf_payload_fits(Fi.len[k])) { ++bo.n_dev; BgzfOut::frame_block(Fi.crc[k], 0xFF00, Fi.payload + k * 0x10000, Fi.len[k], out); }
    else { ++bo.n_declined; if (!BgzfOut::deflate_block(Fi.raw + Fi.raw_at[k], 0xFF00, out, bo.level)) { msg = "cannot write the BAM"; return TRGT_ERR_INVALID; } }
    if (std::fwrite(out.data(), 1, out.size(), bo.f) != out.size()) { msg = "cannot write the BAM"; return TRGT_ERR_INVALID; }
  }
  bo.buf.assign(Fi.tail, Fi.tail + Fi.tail_bytes);
  return TRGT_OK;
}
// a flush and its "[writer]" line: the device path reports the flushes that worked, the host path the ones made inside the call
int run_flush(trgt_writer* w, Flush flush, Pieces& p, std::string& msg) {
  const int rc = flush(w, p, msg);
  if (p.tr.on && (rc == TRGT_OK || !p.tr.device)) trace_line(p.tr, w->bam);
  return rc;
}

// One trgt_writer_write / trgt_writer_write_meth call: what its stages share.  given_meth (trgt_writer_write_meth): Allele::meth per output
// slot, NaN = None, in place of the host's own get_meth over the reads' bases.
struct WriteCall {
  trgt_writer* w; const trgt_ingest_batch* b; const trgt_locus_batch_out* o; const double* given_meth;
  int64_t nl = 0; int nt = 1;  // loci, workers that format them
  double t0 = 0;
  bool trace = false;
  Pieces pcs;
  br::BatchDev D; std::vector<br::RecIn> rin; std::vector<br::LocusIn> lin; std::string ids; br::Assembled A;  // records_device

  int check_args() {
    if (!w || !b || !o) return TRGT_ERR_INVALID;
    if (!o->n_alleles || !o->allele_blob || !o->allele_off || !o->allele_len || !o->ci || !o->num_spanning || !o->classification || !o->read_rank ||
        !o->span_start || !o->span_end || !o->spans3 || !o->span_off || !o->n_spans || !o->motif_counts || !o->count_off || !o->purity) {
      w->err = "trgt_writer_write: incomplete result arrays"; return TRGT_ERR_INVALID;
    }
    return TRGT_OK;
  }
  void size_pieces() {
    static const bool trace_env = std::getenv("TRGT_WRITER_TRACE") != nullptr;
    trace = trace_env; nl = b->n_loci; t0 = now_ms();
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(w->threads, nl / 16));
    pcs.lines.resize((size_t)nt); pcs.errs.resize((size_t)nt); pcs.recs.resize((size_t)nt);
  }
  // every locus by wf::format_locus, worker t the loci [nl * t / nt, nl * (t + 1) / nt); a worker stops at its first failing locus
  void format_all(bool host_records) {
    const wf::FormatCtx c{b, o, given_meth, &w->contigs, w->flank_len, w->keep_unmapped, w->has_bam, host_records};
    auto work = [&](int t) {
      try {
        std::vector<uint8_t> rec;
        for (int64_t l = nl * t / nt; l < nl * (t + 1) / nt; ++l) if (!wf::format_locus(c, l, pcs.lines[(size_t)t], pcs.recs[(size_t)t], rec, pcs.errs[(size_t)t])) return;
      } catch (const std::exception& e) { pcs.errs[(size_t)t] = std::string("trgt_writer_write: ") + e.what(); }
    };
    for (int t = 0; t < nt; ++t) { pcs.lines[(size_t)t].clear(); pcs.errs[(size_t)t].clear(); pcs.recs[(size_t)t].clear(); }
    if (nt <= 1) work(0);
    else { std::vector<std::thread> th; for (int t = 0; t < nt; ++t) th.emplace_back(work, t); for (auto& t : th) t.join(); }
  }
  Trace trace_of(bool device, double t_dev, double t_fmt) const {
    Trace tr; tr.on = trace; tr.device = device; tr.t0 = t0; tr.t_dev = t_dev; tr.t_fmt = t_fmt; tr.nl = nl; tr.nt = nt;
    for (int t = 0; t < nt; ++t) { tr.vcf_bytes += pcs.lines[(size_t)t].size(); tr.rec_bytes += pcs.recs[(size_t)t].size(); }
    return tr;
  }
  // D: the device addresses of the batch's per-read arrays.  false: they do not all lie in the slab the ingestion left on rec_device.
  bool map_device_batch() {
    const void *sd = nullptr, *sp = nullptr; size_t sbytes = 0; int sdev = -1;
    bool mapped = b->read_blob_dev != nullptr && b->read_blob_device == w->rec_device && trgt::ingest_batch_slab(b, &sd, &sp, &sbytes, &sdev) && sdev == w->rec_device;
    auto at = [&](const void* host, auto** out) {  // the device address of an array of the pinned mirror
      const uintptr_t h = (uintptr_t)host, p0 = (uintptr_t)sp;
      if (!host || h < p0 || h >= p0 + sbytes) { mapped = false; return; }
      *out = reinterpret_cast<std::remove_reference_t<decltype(*out)>>((uintptr_t)sd + (h - p0));
    };
    if (!mapped) return false;
    D.n_reads = b->n_reads;
    at(b->read_off, &D.read_off); at(b->read_len, &D.read_len); at(b->read_blob, &D.reads); at(b->qual_blob, &D.quals); at(b->name_blob, &D.names); at(b->name_off, &D.name_off);
    at(b->read_qual, &D.rq); at(b->is_reverse, &D.is_reverse); at(b->mapq, &D.mapq); at(b->hp_tag, &D.hp); at(b->start_offset, &D.start_offset); at(b->end_offset, &D.end_offset);
    at(b->mismatch_offsets, &D.snp); at(b->mismatch_off, &D.snp_off); at(b->meth, &D.meth); at(b->meth_off, &D.meth_off); at(b->has_meth, &D.has_meth); at(b->cigar, &D.cig);
    at(b->cigar_off, &D.cig_off); at(b->cigar_ref_pos, &D.cig_ref_pos);
    return mapped;
  }
  // rin / lin / ids: the kept reads in record order with their results; per locus the contig's tid and the id text.  false: a VCF line
  // failed, a contig is not in the header or a locus's reads are out of range (the host path reports it).
  bool plan_records() {
    for (int t = 0; t < nt; ++t) if (!pcs.errs[(size_t)t].empty()) return false;
    lin.resize((size_t)nl);
    std::vector<uint64_t> kept;
    for (int64_t l = 0; l < nl; ++l) {
      const int tid = wf::contig_tid(w->contigs, b->contig_blob + b->contig_off[l], (size_t)(b->contig_off[l + 1] - b->contig_off[l]));
      if (tid < 0) return false;
      lin[(size_t)l] = br::LocusIn{tid, (uint32_t)ids.size(), (uint32_t)(b->id_off[l + 1] - b->id_off[l])};
      ids.append(b->id_blob + b->id_off[l], b->id_off[l + 1] - b->id_off[l]);
      const uint64_t r0 = b->locus_read_begin[l], r1 = b->locus_read_begin[l + 1];
      if (r1 > (uint64_t)b->n_reads || r0 > r1) return false;
      wf::kept_reads(b, o, l, kept);
      for (uint64_t r : kept) rin.push_back(br::RecIn{(uint32_t)r, (uint32_t)l, o->span_start[r], o->span_end[r], (int32_t)o->classification[r]});
    }
    return true;
  }
  int assemble_on_device() {
    std::string e;
    const int rc = br::assemble(w->rec, D, rin.data(), rin.size(), lin.data(), lin.size(), ids.data(), ids.size(), (uint32_t)w->flank_len, w->keep_unmapped, w->bam.buf.data(),
                                w->bam.buf.size(), A, e);
    if (rc) w->err = "trgt_writer_write: " + e;
    return rc;
  }
  // records_device: the records of a batch whose per-read arrays lie in HBM of that GPU are assembled there (bam_records_dev.hip).
  // host_reason 1 (not such a batch) or 2 (a batch the planner or the kernels flag): nothing was written, the batch goes through the
  // host code.  host_reason 0: the call ends here with rc, handed over or failed.
  struct DeviceVerdict { int host_reason, rc; };
  DeviceVerdict device_records() {
    if (!map_device_batch()) return {1, TRGT_OK};
    format_all(false);  // the VCF lines (host: small, and AM needs the results' doubles)
    if (!plan_records()) return {2, TRGT_OK};
    const double t1 = now_ms();
    if (w->write_behind) { if (const int prc = w->bg_wait()) return {0, prc}; }  // (the tail of the stream is the flush's before this one)
    if (const int arc = assemble_on_device()) return {0, arc};
    if (A.flags) return {2, TRGT_OK};
    ++w->rec_stats[0]; w->rec_stats[3] += (int64_t)A.n_records; w->rec_stats[4] += (int64_t)A.rec_bytes;
    w->bam.link_up += (int64_t)A.h2d_bytes;
    pcs.tr = trace_of(true, t1, now_ms());
    pcs.tr.rec_bytes = A.rec_bytes; pcs.tr.n_records = A.n_records;
    return {0, hand_over(flush_device)};
  }
  // The one way out for the formatted pieces: flushed here, or -- write_behind -- by the writer's thread once the batch before this one
  // is out (one in flight; its verdict is this call's when it failed; this one's comes back from the next write or the close)
  int hand_over(Flush flush) {
    if (!w->write_behind) {
      std::string msg;
      const int rc = run_flush(w, flush, pcs, msg);
      if (rc) w->err = msg;
      return rc;
    }
    if (const int prc = w->bg_wait()) return prc;
    auto own = std::make_shared<Pieces>(std::move(pcs));
    trgt_writer* ww = w;
    w->bg = std::thread([ww, own, flush]() {
      try { std::string msg; ww->bg_rc = run_flush(ww, flush, *own, msg); if (ww->bg_rc != TRGT_OK) ww->bg_err = msg; }
      catch (const std::exception& e) { ww->bg_rc = TRGT_ERR_NOMEM; ww->bg_err = std::string("trgt_writer_write: ") + e.what(); }
    });
    return TRGT_OK;
  }
};

}  // namespace

extern "C" {

const char* trgt_writer_last_error(const trgt_writer* w) { return w ? w->err.c_str() : "null handle"; }
// ABI 10: BGZF blocks of the spanning BAM so far -- out[0] deflated on the device, [1] declined by it (zlib took them), [2] deflated by zlib
// because no device was named or the flush held fewer than 16 full blocks
void trgt_writer_device_stats(const trgt_writer* w, int64_t out[3]) { if (w && out) { out[0] = w->bam.n_dev.load(); out[1] = w->bam.n_declined.load(); out[2] = w->bam.n_host.load(); } }
// the records of device-ingested batches assembled on GPU `device` (bam_records_dev.hip); see include/trgt_hip.h
int trgt_writer_set_records_device(trgt_writer* w, int32_t device) {
  if (!w) return TRGT_ERR_INVALID;
  try {
    auto bad = [&](int rc, const std::string& m) { w->err = m; return rc; };
    if (w->wrote) return bad(TRGT_ERR_INVALID, "trgt_writer_set_records_device: called after the first trgt_writer_write");
    if (device < 0) { if (w->rec) { trgt::brec::engine_destroy(w->rec); w->rec = nullptr; } w->rec_device = -1; return TRGT_OK; }
    if (!w->has_bam) return bad(TRGT_ERR_INVALID, "trgt_writer_set_records_device: records_device " + std::to_string(device) + " on a writer without a spanning BAM");
    if (w->dev && w->dev_ordinal != device)
      return bad(TRGT_ERR_INVALID, "trgt_writer_set_records_device: records_device " + std::to_string(device) + " and deflate_device " + std::to_string(w->dev_ordinal) + " must name the same GPU");
    std::string e;
    int n = 0;
    trgt::brec::Engine* eng = trgt::brec::engine_create(device, e, &n);
    if (!eng) return bad(n <= 0 ? TRGT_ERR_NO_DEVICE : TRGT_ERR_INVALID, "trgt_writer_set_records_device: " + e);
    if (w->rec) trgt::brec::engine_destroy(w->rec);
    w->rec = eng; w->rec_device = device;
    return TRGT_OK;
  } catch (const std::exception& e) { w->err = std::string("trgt_writer_set_records_device: ") + e.what(); return TRGT_ERR_NOMEM; }
}
void trgt_writer_records_stats(const trgt_writer* w, int64_t out[5]) { if (w && out) for (int i = 0; i < 5; ++i) out[i] = w->rec_stats[i].load(); }

void trgt_writer_default_params(trgt_writer_params* p) {
  if (!p) return;
  p->output_flank_len = 50; p->sample_name = "sample"; p->program = "trgt"; p->version = "3.0.0"; p->command_line = ""; p->keep_unmapped_flag = 1; p->threads = 0; p->bam_compress_level = 6; p->deflate_device = -1; p->write_behind = 0;
}

static int writer_open_impl(const trgt_ingest* src, const trgt_writer_params* p, const char* vcf_path, const char* bam_path, trgt_writer** out) {
  if (!src || !p || !vcf_path || !out) return TRGT_ERR_INVALID;
  std::unique_ptr<trgt_writer> w(new trgt_writer());
  *out = nullptr;
  auto bad = [&](const std::string& m) { w->err = m; *out = w.release(); return TRGT_ERR_INVALID; };
  w->flank_len = p->output_flank_len; w->keep_unmapped = p->keep_unmapped_flag != 0;
  w->threads = p->threads > 0 ? p->threads : (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
  w->write_behind = p->write_behind != 0;
  w->vcf.threads = w->bam.threads = w->threads;
  w->bam.level = std::min(9, std::max(0, p->bam_compress_level));
  if (p->deflate_device >= 0 && bam_path) {  // the spanning BAM's blocks on the GPU (the VCF stays with zlib: it is small)
    if (trgt_hip_create(p->deflate_device, &w->dev) != TRGT_OK) { const std::string m = w->dev ? trgt_hip_last_error(w->dev) : "no such device"; if (w->dev) { trgt_hip_destroy(w->dev); w->dev = nullptr; } return bad("deflate_device: " + m); }
    w->bam.dev = w->dev; w->dev_ordinal = p->deflate_device;
  }
  const std::string prog = p->program ? p->program : "trgt", ver = p->version ? p->version : "", cl = p->command_line ? p->command_line : "";
  w->sample = p->sample_name ? p->sample_name : "sample";
  for (int32_t i = 0; i < trgt_ingest_n_contigs(src); ++i) w->contigs.push_back(trgt_ingest_contig_name(src, i));
  if (!w->vcf.open(vcf_path, ends_with(vcf_path, ".gz"))) return bad(std::string("Invalid VCF output path: ") + vcf_path);
  {  // VcfWriter::new (write_vcf.rs:49-92); the first two lines are what htslib puts into every new header
    std::string h = "##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n";
    h += "##INFO=<ID=TRID,Number=1,Type=String,Description=\"Tandem repeat ID\">\n"
         "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant described in this record\">\n"
         "##INFO=<ID=MOTIFS,Number=.,Type=String,Description=\"Motifs that the tandem repeat is composed of\">\n"
         "##INFO=<ID=STRUC,Number=1,Type=String,Description=\"Structure of the region\">\n"
         "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
         "##FORMAT=<ID=AL,Number=.,Type=Integer,Description=\"Length of each allele\">\n"
         "##FORMAT=<ID=ALLR,Number=.,Type=String,Description=\"Length range per allele\">\n"
         "##FORMAT=<ID=SD,Number=.,Type=Integer,Description=\"Number of spanning reads supporting per allele\">\n"
         "##FORMAT=<ID=MC,Number=.,Type=String,Description=\"Motif counts per allele\">\n"
         "##FORMAT=<ID=MS,Number=.,Type=String,Description=\"Motif spans per allele\">\n"
         "##FORMAT=<ID=AP,Number=.,Type=Float,Description=\"Allele purity per allele\">\n"
         "##FORMAT=<ID=AM,Number=.,Type=Float,Description=\"Mean methylation level per allele\">\n";
    for (int32_t i = 0; i < trgt_ingest_n_contigs(src); ++i)
      h += "##contig=<ID=" + w->contigs[(size_t)i] + ",length=" + std::to_string(trgt_ingest_contig_length(src, i)) + ">\n";
    h += "##" + prog + "Version=" + ver + "\n##" + prog + "Command=" + cl + "\n";
    h += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + w->sample + "\n";
    if (!w->vcf.write(h.data(), h.size())) return bad("cannot write the VCF header");
  }
  if (bam_path) {
    if (!w->bam.open(bam_path, true)) return bad(std::string("cannot open ") + bam_path);
    w->has_bam = true;
    std::string text = trgt_ingest_header_text(src);  // BamWriter::create_header (write_bam.rs:52-65): the template + a @PG record
    if (!text.empty() && text.back() != '\n') text += "\n";
    text += "@PG\tID:" + prog + "\tPN:" + prog + "\tCL:" + cl + "\tVN:" + ver + "\n";
    std::vector<uint8_t> h = {'B', 'A', 'M', 1};
    put32(h, (uint32_t)text.size()); h.insert(h.end(), text.begin(), text.end());
    put32(h, (uint32_t)w->contigs.size());
    for (size_t i = 0; i < w->contigs.size(); ++i) {
      put32(h, (uint32_t)w->contigs[i].size() + 1); h.insert(h.end(), w->contigs[i].begin(), w->contigs[i].end()); h.push_back(0);
      put32(h, trgt_ingest_contig_length(src, (int32_t)i));
    }
    if (!w->bam.write(h.data(), h.size())) return bad("cannot write the BAM header");
  }
  *out = w.release();
  return TRGT_OK;
}

// The stages of a write, top to bottom (WriteCall above; the formatting itself is writer_format.hpp)
static int writer_write_impl(trgt_writer* w, const trgt_ingest_batch* b, const trgt_locus_batch_out* o, const double* given_meth = nullptr) {
  WriteCall c{w, b, o, given_meth};
  if (const int rc = c.check_args()) return rc;
  w->wrote = true;
  c.size_pieces();
  if (w->rec && w->has_bam) {
    const WriteCall::DeviceVerdict v = c.device_records();
    if (!v.host_reason) return v.rc;
    ++w->rec_stats[1]; w->rec_stats[2] = v.host_reason;  // any other batch, and a batch the kernels flag, is formatted below and counted with its reason
    c.t0 = now_ms();
  }
  c.format_all(true);
  c.pcs.tr = c.trace_of(false, 0, now_ms());
  c.pcs.tr.on = c.trace && !w->write_behind;  // (behind the call the line would time the hand-over, not the flush)
  return c.hand_over(flush_pieces);
}

// HiFiRead::clip_bases on its own (include/trgt_hip.h: "per-read helpers")
int64_t trgt_read_clip_bases(const uint8_t* bases, const uint8_t* quals, int64_t n_bases, const uint8_t* meth, int64_t n_meth, const uint32_t* cigar,
                             int64_t n_ops, int64_t ref_pos, int64_t left_len, int64_t right_len, uint8_t* out_bases, uint8_t* out_quals,
                             uint8_t* out_meth, int64_t* out_meth_n, uint32_t* out_cigar, int64_t* out_n_ops, int64_t* out_ref_pos) {
  if (n_bases < 0 || (n_bases > 0 && (!bases || !quals || !out_bases || !out_quals)) || n_ops < 0 || (n_ops > 0 && !cigar) || !out_cigar || !out_n_ops ||
      !out_ref_pos || !out_meth_n || (n_meth > 0 && (!meth || !out_meth)) || left_len < 0 || right_len < 0)
    return TRGT_ERR_INVALID;
  try {
    if (left_len + right_len >= n_bases) return -1;  // clip_bases.rs:10-12
    const size_t left = (size_t)left_len, right = (size_t)right_len, n = (size_t)n_bases, len = n - left - right;
    std::vector<uint32_t> ops; int64_t rp = ref_pos;
    if (!wf::clip_bases_cigar(cigar, (size_t)n_ops, left, right, ops, rp)) return TRGT_ERR_INVALID;
    std::memcpy(out_bases, bases + left, len); std::memcpy(out_quals, quals + left, len);
    *out_meth_n = -1;
    if (n_meth >= 0) { std::vector<uint8_t> m; wf::clip_bases_meth(bases, n, meth, (size_t)n_meth, left, right, m); std::copy(m.begin(), m.end(), out_meth); *out_meth_n = (int64_t)m.size(); }
    std::copy(ops.begin(), ops.end(), out_cigar); *out_n_ops = (int64_t)ops.size(); *out_ref_pos = rp;
    return (int64_t)len;
  } catch (const std::exception&) { return TRGT_ERR_NOMEM; }
}

int trgt_writer_open(const trgt_ingest* src, const trgt_writer_params* p, const char* vcf_path, const char* bam_path, trgt_writer** out) {
  try { return writer_open_impl(src, p, vcf_path, bam_path, out); } catch (const std::exception&) { return TRGT_ERR_NOMEM; }  // (exceptions never cross the C ABI)
}
int trgt_writer_write(trgt_writer* w, const trgt_ingest_batch* b, const trgt_locus_batch_out* o) {
  try { return writer_write_impl(w, b, o); } catch (const std::exception& e) { if (w) w->err = std::string("trgt_writer_write: ") + e.what(); return TRGT_ERR_NOMEM; }
}
int trgt_writer_write_meth(trgt_writer* w, const trgt_ingest_batch* b, const trgt_locus_batch_out* o, const double* allele_meth, const int32_t* meth_reads) {
  if (!w) return TRGT_ERR_INVALID;
  if (!allele_meth || !meth_reads) { w->err = "trgt_writer_write_meth: allele_meth and meth_reads are both required"; return TRGT_ERR_INVALID; }
  try { return writer_write_impl(w, b, o, allele_meth); } catch (const std::exception& e) { w->err = std::string("trgt_writer_write_meth: ") + e.what(); return TRGT_ERR_NOMEM; }
}

int trgt_writer_close(trgt_writer* w) {
  if (!w) return TRGT_OK;
  const int brc = w->bg_wait();  // (write_behind: the last batch's pieces)
  const bool ok1 = w->vcf.close(), ok2 = !w->has_bam || w->bam.close();
  delete w;
  return brc != TRGT_OK ? brc : ok1 && ok2 ? TRGT_OK : TRGT_ERR_INVALID;
}

}  // extern "C"
