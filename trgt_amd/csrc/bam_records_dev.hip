// trgt_amd/csrc/bam_records_dev.hip -- the spanning-BAM records of a batch assembled on the device from the per-read arrays the device
// ingestion left in HBM (ingest_dev.hip's slab), for the writer (writers.hip, trgt_writer_set_records_device):
//   BamWriter::write       src/trgt/writers/write_bam.rs:72-144   the record: head, name, CIGAR, 4-bit bases, qualities, tags TR rq MC MO HP SO EO AL FL
//   HiFiRead::clip_bases   src/trgt/reads/clip_bases.rs:9-120     bases / qualities / per-CpG methylation / CIGAR without the first `left` and last `right` bases
//
//   sizes_kernel   one wave per kept read: the skip rules, clip_cigar as prefix sums over 64 operations a step, the CpGs before and inside
//                  the kept bases, the record's size; a result or an array that does not fit the read's own lengths raises a flag
//   scan_kernel    exclusive sums of the sizes in record order -> where every record starts in the stream
//   fill_kernel    one workgroup (a wave) per record writes it: dword stores wherever four bytes of the stream are aligned, byte stores at the edges
// The stream is the writer's carried tail (less than one BGZF block, uploaded) followed by the records; finish() has its full 0xFF00-byte
// blocks checksummed (crc32_blocks_kernel of ingest_dev.hip) and deflated (deflate_dev.hip) where they lie and brings back payloads,
// lengths, CRCs and the tail -- or, without a deflate device, the stream itself for zlib.  The record bytes are what writer_format.hpp's
// bam_record produces, byte for byte; the three errors it reports are flags here and the host path redoes such a batch.
#include <cmath>
#include <cstring>
#include <memory>

#include "common.hpp"
#include "bam_records_dev.hpp"
#include "bgzf_block.hpp"
#include "ingest_dev.hpp"

namespace trgt {
int deflate_device_blocks_ff00(trgt_hip_ctx* c, int64_t n, const uint8_t* d_src, uint8_t* dst, uint64_t slot, uint32_t cap, uint32_t* dst_len);  // deflate_dev.hip

namespace brec {

// sizes_kernel -> fill_kernel
struct RecInfo {
  uint32_t size;               // bytes of the record with its block_size word; 0 = no record (a skip rule, or a flag)
  uint32_t left, len;          // bases dropped in front, bases kept
  uint32_t i0, n_ops;          // first operation kept (whole or in part), operations kept
  uint32_t keep;               // query bases the kept operations cover
  uint32_t meth_first, meth_n; // first per-CpG value kept, values kept
  uint64_t q0;                 // query bases of the operations before i0
  int64_t ref_pos, ref_end;
};
struct Totals { uint64_t bytes, records; uint32_t flags, pad; };

__device__ __forceinline__ int lane_id() { return (int)threadIdx.x & 63; }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) { return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src); }
__device__ __forceinline__ uint64_t wave_incl_sum(uint64_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint64_t o = shfl64(v, lane - d < 0 ? lane : lane - d); if (lane >= d) v += o; }
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) { return shfl64(wave_incl_sum(v), 63); }
__device__ __forceinline__ uint32_t qry_len(uint32_t op) { const uint32_t c = op & 0xFu; return (c == 0 || c == 1 || c == 4 || c == 7 || c == 8) ? op >> 4 : 0u; }
__device__ __forceinline__ bool takes_ref(uint32_t op) { const uint32_t c = op & 0xFu; return c == 0 || c == 2 || c == 3 || c == 7 || c == 8; }
// little-endian word at any alignment: two aligned loads (every array of the slab is a 64-byte aligned piece with slack behind it)
__device__ __forceinline__ uint32_t uld32(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3u) * 8u;
  const uint32_t lo = q[0];
  if (!sh) return lo;
  return (lo >> sh) | (q[1] << (32u - sh));
}
__device__ __forceinline__ void st32(uint8_t* p, uint32_t v) {
  if (((uintptr_t)p & 3u) == 0) { *(uint32_t*)p = v; return; }
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
__device__ __forceinline__ uint32_t nib_of(uint32_t c) {  // "=ACMGRSVTWYHKDBN", anything else 15
  switch (c) { case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
               case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14; default: return 15; }
}
__device__ __forceinline__ int reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// One operation of the clipped CIGAR (clip_bases.rs:59-118).  excl / incl: query bases before / through the operation in the unclipped read.
// Operations with excl < left and incl <= left are dropped whole (clip_cigar's first loop stops the moment `left` bases are gone: an
// operation without query bases AT the cut stays); then operations are kept while fewer than `keep` bases are out, the last one cut short.
__device__ __forceinline__ uint32_t clipped_op(uint32_t op, uint64_t excl, uint64_t incl, uint64_t left, uint64_t keep) {
  if (qry_len(op) == 0) return op;
  const uint64_t s = (excl > left ? excl : left) - left, e = incl - left;
  return ((uint32_t)((e < keep ? e : keep) - s) << 4) | (op & 0xFu);
}

// ------------------------------------------------------------------------------------------------ sizes
__global__ void __launch_bounds__(64) sizes_kernel(BatchDev B, const RecIn* __restrict__ recs, uint32_t n_recs, const LocusIn* __restrict__ loci, uint32_t n_loci, uint32_t F,
                                                   RecInfo* __restrict__ info, Totals* __restrict__ totals) {
  const uint32_t k = blockIdx.x;
  if (k >= n_recs) return;
  const int lane = lane_id();
  RecInfo I; memset(&I, 0, sizeof I);
  auto leave = [&](uint32_t flag) { if (lane == 0) { if (flag) atomicOr(&totals->flags, flag); I.size = 0; info[k] = I; } };
  const RecIn R = recs[k];
  if ((int64_t)R.read >= B.n_reads || R.locus >= n_loci || R.span_start < 0 || R.span_end < 0) return leave(FLAG_RANGE);
  const uint64_t r = R.read;
  const uint64_t s0 = (uint64_t)R.span_start, s1 = (uint64_t)R.span_end, n = B.read_len[r];
  if (s0 < F || n < s1 + F) return leave(0);      // "unexpectedly short flanks" (write_bam.rs)
  const uint64_t left = s0 - F, right = n - s1 - F;
  if (left + right >= n) return leave(0);         // clip_bases: None
  const uint64_t len = n - left - right;
  // ---- clip_cigar: the query bases of all operations, then the cut
  const uint64_t c0 = B.cig_off[r], c1 = B.cig_off[r + 1], nm0 = B.name_off[r], nm1 = B.name_off[r + 1], sn0 = B.snp_off[r], sn1 = B.snp_off[r + 1];
  if (c1 < c0 || c1 - c0 > 0x7FFFFFFFull || nm1 < nm0 || sn1 < sn0 || nm1 - nm0 > 0xFFFFFFull || sn1 - sn0 > 0xFFFFFFull) return leave(FLAG_RANGE);
  const uint32_t nc = (uint32_t)(c1 - c0);
  const uint32_t* cg = B.cig + c0;
  uint64_t qsum = 0;
  for (uint32_t base = 0; base < nc; base += 64) { const uint32_t i = base + (uint32_t)lane; qsum += i < nc ? qry_len(cg[i]) : 0u; }
  qsum = wave_sum(qsum);
  if (qsum < left + right) return leave(FLAG_CIGAR_SHORT);
  const uint64_t keep = qsum - left - right;
  uint64_t carry = 0, ref_add = 0, end_add = 0, n_ops = 0, q0 = 0;
  uint32_t i0 = nc; bool have_i0 = false;
  for (uint32_t base = 0; base < nc; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    const bool valid = i < nc;
    const uint32_t op = valid ? cg[i] : 0u, q = qry_len(op);
    const uint64_t incl = wave_incl_sum(q) + carry, excl = incl - q;
    const bool dropped = valid && excl < left && incl <= left;
    const bool cand = valid && !dropped;
    if (dropped && takes_ref(op)) ref_add += op >> 4;
    if (cand && excl < left && takes_ref(op)) ref_add += left - excl;     // the first kept operation, cut in front
    const uint64_t s = (excl > left ? excl : left) - left;
    if (cand && s < keep) { ++n_ops; if (takes_ref(op)) end_add += clipped_op(op, excl, incl, left, keep) >> 4; }
    const uint64_t m = __ballot(cand);
    if (!have_i0 && m) { const int f = __ffsll((long long)m) - 1; i0 = base + (uint32_t)f; q0 = shfl64(excl, f); have_i0 = true; }
    carry = shfl64(incl, 63);
  }
  ref_add = wave_sum(ref_add); end_add = wave_sum(end_add); n_ops = wave_sum(n_ops);
  if (n_ops > 65535) return leave(FLAG_CIGAR_OPS);
  // ---- clip_bases' methylation: per-CpG values of the CpGs whose C lies in [left, n - right); `first` CpGs lie before
  uint32_t meth_first = 0, meth_n = 0;
  const bool hm = B.has_meth[r] != 0;
  if (hm) {
    const uint64_t m0 = B.meth_off[r], m1 = B.meth_off[r + 1];
    if (m1 < m0) return leave(FLAG_RANGE);
    const uint64_t nme = m1 - m0, hi = n - right;           // a C at idx counts when idx < hi and idx + 1 < n
    const uint64_t lim = hi + 1 < n ? hi + 1 : n;           // bytes [0, lim) of the read are looked at
    const uint8_t* p = B.reads + B.read_off[r];
    const uint32_t a = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* pw = (const uint32_t*)(p - a);
    const uint64_t n_words = (a + lim + 3) / 4;
    uint64_t before = 0, inside = 0;
    for (uint64_t j = (uint64_t)lane; j < n_words; j += 64) {
      const uint32_t w0 = pw[j], w1 = j + 1 < n_words ? pw[j + 1] : 0u;
      const uint64_t w = (uint64_t)w0 | ((uint64_t)w1 << 32);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t idx = (int64_t)(4 * j) + t - (int64_t)a;
        const bool cpg = ((w >> (8 * t)) & 0xFFFFu) == (uint32_t)('C' | ('G' << 8)) && idx >= 0 && (uint64_t)idx < hi && (uint64_t)idx + 1 < n;
        if (cpg) { if ((uint64_t)idx < left) ++before; else ++inside; }
      }
    }
    before = wave_sum(before); inside = wave_sum(inside);
    if (before < nme) { meth_first = (uint32_t)before; meth_n = (uint32_t)((before + inside < nme ? before + inside : nme) - before); }   // (ci < nme)
  }
  const uint64_t size = 36ull + (nm1 - nm0) + 1 + 4 * n_ops + (len + 1) / 2 + len + (4ull + loci[R.locus].id_len) + 7 + (hm ? 8ull + meth_n : 0ull) + 8 + 4 * (sn1 - sn0) +
                        (B.hp[r] >= 0 ? 4u : 0u) + 21 + 16;
  if (size >= (1ull << 31)) return leave(FLAG_RANGE);
  if (lane == 0) {
    I.size = (uint32_t)size; I.left = (uint32_t)left; I.len = (uint32_t)len; I.i0 = i0; I.n_ops = (uint32_t)n_ops; I.keep = (uint32_t)keep; I.meth_first = meth_first; I.meth_n = meth_n; I.q0 = q0;
    I.ref_pos = B.cig_ref_pos[r] + (int64_t)ref_add; I.ref_end = I.ref_pos + (int64_t)end_add;
    info[k] = I;
  }
}

// ------------------------------------------------------------------------------------------------ where every record starts
// One workgroup: thread t sums a contiguous run of records, the runs' sums are scanned, the run is walked again (ingest_dev.hip's scan_kernel).
__global__ void __launch_bounds__(1024) scan_kernel(const RecInfo* __restrict__ info, uint32_t n_recs, uint64_t* __restrict__ off, Totals* __restrict__ totals) {
  __shared__ uint64_t part[1024][2];
  const uint32_t t = threadIdx.x;
  const uint32_t run = (n_recs + 1023) / 1024, a = min(n_recs, t * run), b = min(n_recs, a + run);
  uint64_t bytes = 0, cnt = 0;
  for (uint32_t i = a; i < b; ++i) { const uint32_t s = info[i].size; bytes += s; cnt += s != 0; }
  part[t][0] = bytes; part[t][1] = cnt;
  __syncthreads();
  if (t < 2) { uint64_t acc = 0; for (int i = 0; i < 1024; ++i) { const uint64_t v = part[i][t]; part[i][t] = acc; acc += v; } if (t == 0) totals->bytes = acc; else totals->records = acc; }
  __syncthreads();
  uint64_t acc = part[t][0];
  for (uint32_t i = a; i < b; ++i) { off[i] = acc; acc += info[i].size; }
}

// ------------------------------------------------------------------------------------------------ the records
// `n` bytes at d, of which the first n_full may go out as words: byte_at(j) / word_at(j) give the byte / the four bytes at offset j.
// Bytes until d + j is 4-aligned and behind the last whole word are byte stores, the rest dword stores (64 lanes: 256 contiguous bytes a step).
template <class FB, class FW>
__device__ __forceinline__ void put_seg(uint8_t* d, uint32_t n, uint32_t n_full, int lane, FB byte_at, FW word_at) {
  uint32_t head = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
  if (head > n_full) head = n_full;
  const uint32_t words = (n_full - head) / 4, tail0 = head + 4 * words;
  for (uint32_t j = (uint32_t)lane; j < head; j += 64) d[j] = byte_at(j);
  for (uint32_t w = (uint32_t)lane; w < words; w += 64) *(uint32_t*)(d + head + 4 * w) = word_at(head + 4 * w);
  for (uint32_t j = tail0 + (uint32_t)lane; j < n; j += 64) d[j] = byte_at(j);
}

__global__ void __launch_bounds__(64) fill_kernel(BatchDev B, const RecIn* __restrict__ recs, uint32_t n_recs, const LocusIn* __restrict__ loci, const char* __restrict__ id_blob, uint32_t F,
                                                  uint32_t flag_base, const RecInfo* __restrict__ info, const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
  __shared__ uint8_t nib[256];
  const uint32_t k = blockIdx.x;
  if (k >= n_recs) return;
  const int lane = lane_id();
  const RecInfo I = info[k];
  if (!I.size) return;
  for (int c = lane; c < 256; c += 64) nib[c] = (uint8_t)nib_of((uint32_t)c);
  __syncthreads();
  const RecIn R = recs[k];
  const uint64_t r = R.read;
  const LocusIn L = loci[R.locus];
  uint8_t* const d = out + off[k];
  const uint64_t nm0 = B.name_off[r], sn0 = B.snp_off[r];
  const uint32_t n_name = (uint32_t)(B.name_off[r + 1] - nm0), n_snp = (uint32_t)(B.snp_off[r + 1] - sn0);
  const uint32_t o_cig = 36 + n_name + 1, o_seq = o_cig + 4 * I.n_ops, o_qual = o_seq + (I.len + 1) / 2, o_tag = o_qual + I.len;
  // ---- head (write_bam.rs:96-111; the mate fields as rust-htslib's Record::new leaves them), one word per lane
  if (lane < 9) {
    uint32_t v = 0;
    switch (lane) {
      case 0: v = I.size - 4; break;
      case 1: v = (uint32_t)L.tid; break;
      case 2: v = (uint32_t)I.ref_pos; break;
      case 3: v = ((n_name + 1) & 0xFFu) | ((uint32_t)B.mapq[r] << 8) | (((uint32_t)reg2bin(I.ref_pos, I.ref_end > I.ref_pos ? I.ref_end : I.ref_pos + 1) & 0xFFFFu) << 16); break;
      case 4: v = I.n_ops | (((B.is_reverse[r] ? 0x10u : 0u) | flag_base) << 16); break;
      case 5: v = I.len; break;
      case 6: case 7: v = 0xFFFFFFFFu; break;
      default: v = 0; break;
    }
    st32(d + 4 * lane, v);
  }
  { const char* nm = B.names + nm0; for (uint32_t j = (uint32_t)lane; j <= n_name; j += 64) d[36 + j] = j < n_name ? (uint8_t)nm[j] : (uint8_t)0; }
  // ---- CIGAR: the walk of sizes_kernel from the first kept operation
  {
    const uint32_t* cg = B.cig + B.cig_off[r];
    uint64_t carry = I.q0;
    for (uint32_t base = 0; base < I.n_ops; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      const bool valid = i < I.n_ops;
      const uint32_t op = valid ? cg[I.i0 + i] : 0u, q = qry_len(op);
      const uint64_t incl = wave_incl_sum(q) + carry;
      if (valid) st32(d + o_cig + 4 * i, clipped_op(op, incl - q, incl, I.left, I.keep));
      carry = shfl64(incl, 63);
    }
  }
  // ---- bases as 4-bit codes (8 bases -> one word), qualities
  {
    const uint8_t* bs = B.reads + B.read_off[r] + I.left;
    const uint32_t len = I.len;
    auto seq_byte = [&](uint32_t j) -> uint8_t { return (uint8_t)((nib[bs[2 * j]] << 4) | (2 * j + 1 < len ? nib[bs[2 * j + 1]] : 0)); };
    auto seq_word = [&](uint32_t j) -> uint32_t {
      const uint32_t lo = uld32(bs + 2 * j), hi = uld32(bs + 2 * j + 4);
      return ((uint32_t)nib[lo & 0xFFu] << 4) | nib[(lo >> 8) & 0xFFu] | ((uint32_t)nib[(lo >> 16) & 0xFFu] << 12) | ((uint32_t)nib[lo >> 24] << 8) |
             ((uint32_t)nib[hi & 0xFFu] << 20) | ((uint32_t)nib[(hi >> 8) & 0xFFu] << 16) | ((uint32_t)nib[(hi >> 16) & 0xFFu] << 28) | ((uint32_t)nib[hi >> 24] << 24);
    };
    put_seg(d + o_seq, (len + 1) / 2, len / 2, lane, seq_byte, seq_word);
    const uint8_t* qs = B.quals + B.read_off[r] + I.left;
    put_seg(d + o_qual, len, len, lane, [&](uint32_t j) -> uint8_t { return qs[j]; }, [&](uint32_t j) -> uint32_t { return uld32(qs + j); });
  }
  // ---- tags TR rq [MC] MO [HP] SO EO AL FL: a lane per tag's fixed bytes, all lanes on the arrays
  {
    const bool hm = B.has_meth[r] != 0;
    const int hp = B.hp[r];
    const uint32_t p_tr = o_tag, p_rq = p_tr + 4 + L.id_len, p_mc = p_rq + 7, p_mo = p_mc + (hm ? 8 + I.meth_n : 0), p_hp = p_mo + 8 + 4 * n_snp, p_so = p_hp + (hp >= 0 ? 4 : 0),
                   p_eo = p_so + 7, p_al = p_eo + 7, p_fl = p_al + 7;
    auto tag = [&](uint32_t p, char a, char b, char ty) { d[p] = (uint8_t)a; d[p + 1] = (uint8_t)b; d[p + 2] = (uint8_t)ty; };
    if (lane == 0) { tag(p_tr, 'T', 'R', 'Z'); d[p_tr + 3 + L.id_len] = 0; }
    if (lane == 1) { tag(p_rq, 'r', 'q', 'f'); const double q = B.rq[r]; st32(d + p_rq + 3, __float_as_uint(q != q ? -1.0f : (float)q)); }
    if (lane == 2 && hm) { tag(p_mc, 'M', 'C', 'B'); d[p_mc + 3] = 'C'; st32(d + p_mc + 4, I.meth_n); }
    if (lane == 3) { tag(p_mo, 'M', 'O', 'B'); d[p_mo + 3] = 'i'; st32(d + p_mo + 4, n_snp); }
    if (lane == 4 && hp >= 0) { tag(p_hp, 'H', 'P', 'C'); d[p_hp + 3] = (uint8_t)hp; }
    if (lane == 5) { tag(p_so, 'S', 'O', 'i'); st32(d + p_so + 3, (uint32_t)B.start_offset[r]); }
    if (lane == 6) { tag(p_eo, 'E', 'O', 'i'); st32(d + p_eo + 3, (uint32_t)B.end_offset[r]); }
    if (lane == 7) { tag(p_al, 'A', 'L', 'i'); st32(d + p_al + 3, (uint32_t)R.classification); }
    if (lane == 8) { tag(p_fl, 'F', 'L', 'B'); d[p_fl + 3] = 'I'; st32(d + p_fl + 4, 2u); st32(d + p_fl + 8, F); st32(d + p_fl + 12, F); }
    { const char* id = id_blob + L.id_off; for (uint32_t j = (uint32_t)lane; j < L.id_len; j += 64) d[p_tr + 3 + j] = (uint8_t)id[j]; }
    if (hm) { const uint8_t* me = B.meth + B.meth_off[r] + I.meth_first; for (uint32_t j = (uint32_t)lane; j < I.meth_n; j += 64) d[p_mc + 8 + j] = me[j]; }
    { const int32_t* sn = B.snp + sn0; for (uint32_t j = (uint32_t)lane; j < n_snp; j += 64) st32(d + p_mo + 8 + 4 * j, (uint32_t)sn[j]); }
  }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
struct DevBuf {
  void* p = nullptr; size_t cap = 0;
  bool need(size_t bytes) {
    if (cap >= bytes) return true;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
    cap = want;
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
struct PinBuf {
  void* p = nullptr; size_t cap = 0;
  bool need(size_t bytes) {
    if (cap >= bytes) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
    cap = want;
    return true;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
constexpr uint64_t BLOCK = 0xFF00, DEV_SLOT = 0x10000;
constexpr uint32_t DEV_CAP = 0xFF00;
}  // namespace

class Engine {
 public:
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;   // blocking-sync: the caller sleeps while the kernels run (ingest_dev.hip's Slot)
  DevBuf d_up, d_info, d_off, d_totals, d_stream, d_tab, d_desc, d_crc;
  PinBuf up_pin, dn_pin;
  bool tab_ready = false;
  uint64_t stream_bytes = 0;
  std::vector<uint64_t> raw_at;
  ~Engine() {
    if (device >= 0) (void)hipSetDevice(device);
    for (DevBuf* b : {&d_up, &d_info, &d_off, &d_totals, &d_stream, &d_tab, &d_desc, &d_crc}) b->release();
    up_pin.release(); dn_pin.release();
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
  }
  hipError_t wait() { const hipError_t e = hipEventRecord(done, stream); return e != hipSuccess ? e : hipEventSynchronize(done); }
};

Engine* engine_create(int device, std::string& err, int* n_devices) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  *n_devices = n;
  if (n <= 0) { err = "records_device " + std::to_string(device) + ": no HIP device visible (the records are not assembled on the host instead)"; return nullptr; }
  if (device < 0 || device >= n) { err = "records_device " + std::to_string(device) + ": no such GPU"; return nullptr; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { (void)hipGetLastError(); err = "records_device " + std::to_string(device) + " is not a gfx950 GPU"; return nullptr; }
  (void)hipSetDevice(device);
  std::unique_ptr<Engine> e(new Engine());
  e->device = device;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); err = "records_device: hipStreamCreate failed"; return nullptr; }
  if (hipEventCreateWithFlags(&e->done, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); err = "records_device: hipEventCreate failed"; return nullptr; }
  return e.release();
}
void engine_destroy(Engine* e) { delete e; }

#define REC_TRY(expr)                                                                                                          \
  do {                                                                                                                          \
    hipError_t e__ = (expr);                                                                                                    \
    if (e__ != hipSuccess) { err = std::string("records_device: ") + #expr + " failed: " + hipGetErrorString(e__); return TRGT_ERR_HIP; } \
  } while (0)
#define REC_NEED(buf, bytes) do { if (!(buf).need(bytes)) { err = "records_device: out of memory"; return TRGT_ERR_NOMEM; } } while (0)

int assemble(Engine* e, const BatchDev& b, const RecIn* recs, size_t n_recs, const LocusIn* loci, size_t n_loci, const char* id_blob, size_t id_bytes,
             uint32_t flank, bool keep_unmapped, const uint8_t* tail, size_t tail_len, Assembled& out, std::string& err) {
  out = Assembled();
  if (n_recs >= (1ull << 31) || n_loci >= (1ull << 31)) { err = "records_device: batch too large"; return TRGT_ERR_INVALID; }
  REC_TRY(hipSetDevice(e->device));
  hipStream_t st = e->stream;
  e->stream_bytes = 0;
  // ---- upload: kept reads with their results, loci, id text (one pinned staging buffer, one copy)
  auto r64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t a_recs = 0, a_loci = a_recs + r64(n_recs * sizeof(RecIn)), a_ids = a_loci + r64(n_loci * sizeof(LocusIn)), up_bytes = a_ids + r64(id_bytes + 1);
  REC_NEED(e->up_pin, up_bytes + r64(tail_len) + 64); REC_NEED(e->d_up, up_bytes + 64); REC_NEED(e->d_info, (n_recs + 1) * sizeof(RecInfo)); REC_NEED(e->d_off, (n_recs + 1) * 8);
  REC_NEED(e->d_totals, sizeof(Totals));
  uint8_t* up = (uint8_t*)e->up_pin.p;
  if (n_recs) std::memcpy(up + a_recs, recs, n_recs * sizeof(RecIn));
  if (n_loci) std::memcpy(up + a_loci, loci, n_loci * sizeof(LocusIn));
  if (id_bytes) std::memcpy(up + a_ids, id_blob, id_bytes);
  if (tail_len) std::memcpy(up + up_bytes, tail, tail_len);
  REC_TRY(hipMemcpyAsync(e->d_up.p, up, up_bytes, hipMemcpyHostToDevice, st));
  REC_TRY(hipMemsetAsync(e->d_totals.p, 0, sizeof(Totals), st));
  const uint8_t* D = (const uint8_t*)e->d_up.p;
  const RecIn* d_recs = (const RecIn*)(D + a_recs); const LocusIn* d_loci = (const LocusIn*)(D + a_loci); const char* d_ids = (const char*)(D + a_ids);
  if (n_recs) {
    hipLaunchKernelGGL(sizes_kernel, dim3((unsigned)n_recs), dim3(64), 0, st, b, d_recs, (uint32_t)n_recs, d_loci, (uint32_t)n_loci, flank, (RecInfo*)e->d_info.p, (Totals*)e->d_totals.p);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, (const RecInfo*)e->d_info.p, (uint32_t)n_recs, (uint64_t*)e->d_off.p, (Totals*)e->d_totals.p);
    REC_TRY(hipGetLastError());
  }
  REC_NEED(e->dn_pin, 4096);
  Totals* T = (Totals*)e->dn_pin.p;
  REC_TRY(hipMemcpyAsync(T, e->d_totals.p, sizeof(Totals), hipMemcpyDeviceToHost, st));
  REC_TRY(e->wait());
  out.flags = T->flags; out.h2d_bytes = up_bytes;
  if (T->flags) return TRGT_OK;
  out.n_records = T->records; out.rec_bytes = T->bytes; out.stream_bytes = tail_len + T->bytes;
  // ---- the stream: carried tail, then the records
  REC_NEED(e->d_stream, out.stream_bytes + 256);
  if (tail_len) REC_TRY(hipMemcpyAsync(e->d_stream.p, up + up_bytes, tail_len, hipMemcpyHostToDevice, st));
  if (n_recs && T->bytes)
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)n_recs), dim3(64), 0, st, b, d_recs, (uint32_t)n_recs, d_loci, d_ids, flank, keep_unmapped ? 0x4u : 0u, (const RecInfo*)e->d_info.p,
                       (const uint64_t*)e->d_off.p, (uint8_t*)e->d_stream.p + tail_len);
  REC_TRY(hipGetLastError());
  REC_TRY(e->wait());
  out.h2d_bytes += tail_len;
  e->stream_bytes = out.stream_bytes;
  return TRGT_OK;
}

int finish(Engine* e, trgt_hip_ctx* defl, uint64_t min_dev_blocks, Finished& out, std::string& err) {
  out = Finished();
  REC_TRY(hipSetDevice(e->device));
  hipStream_t st = e->stream;
  const uint64_t total = e->stream_bytes, nb = total / BLOCK, tail_len = total - nb * BLOCK;
  out.n_blocks = nb;
  const uint8_t* S = (const uint8_t*)e->d_stream.p;
  if (!defl || nb < min_dev_blocks) {  // zlib takes the blocks: the stream comes back as it is
    REC_NEED(e->dn_pin, total + 64);
    if (total) { REC_TRY(hipMemcpyAsync(e->dn_pin.p, S, total, hipMemcpyDeviceToHost, st)); REC_TRY(e->wait()); }
    out.raw = (const uint8_t*)e->dn_pin.p; out.raw_bytes = total; out.d2h_bytes = total;
    return TRGT_OK;
  }
  if (defl->device != e->device) { err = "records_device: the deflate context is on another GPU"; return TRGT_ERR_INVALID; }
  // ---- CRC-32 of the full blocks where they lie
  if (!e->tab_ready) {
    REC_NEED(e->d_tab, ingd::crc32_tables_bytes());
    std::vector<uint8_t> T(ingd::crc32_tables_bytes()); ingd::crc32_tables_make(T.data());
    REC_TRY(hipMemcpy(e->d_tab.p, T.data(), T.size(), hipMemcpyHostToDevice));
    e->tab_ready = true;
  }
  auto r64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t a_desc = 0, a_crc = a_desc + r64(nb * sizeof(infl::BlockDesc)), a_len = a_crc + r64(nb * 4), a_tail = a_len + r64(nb * 4), a_pay = a_tail + r64(tail_len + 1),
               a_raw = a_pay + r64(nb * DEV_SLOT + 64);
  REC_NEED(e->dn_pin, a_raw + 64); REC_NEED(e->d_desc, nb * sizeof(infl::BlockDesc) + 64); REC_NEED(e->d_crc, nb * 4 + 64);
  uint8_t* P = (uint8_t*)e->dn_pin.p;
  infl::BlockDesc* desc = (infl::BlockDesc*)(P + a_desc);
  for (uint64_t k = 0; k < nb; ++k) desc[k] = infl::BlockDesc{0, k * BLOCK, 0, (uint32_t)BLOCK};
  REC_TRY(hipMemcpyAsync(e->d_desc.p, desc, nb * sizeof(infl::BlockDesc), hipMemcpyHostToDevice, st));
  ingd::crc32_blocks_launch((void*)st, S, (const infl::BlockDesc*)e->d_desc.p, (uint32_t)nb, e->d_tab.p, (uint32_t*)e->d_crc.p);
  REC_TRY(hipGetLastError());
  REC_TRY(hipMemcpyAsync(P + a_crc, e->d_crc.p, nb * 4, hipMemcpyDeviceToHost, st));
  if (tail_len) REC_TRY(hipMemcpyAsync(P + a_tail, S + nb * BLOCK, tail_len, hipMemcpyDeviceToHost, st));
  // ---- deflate (the context's own stream: the assembly is complete, the CRC kernel only reads)
  uint32_t* len = (uint32_t*)(P + a_len);
  if (const int rc = trgt::deflate_device_blocks_ff00(defl, (int64_t)nb, S, P + a_pay, DEV_SLOT, DEV_CAP, len)) { err = std::string("deflate_device: ") + trgt_hip_last_error(defl); return rc; }
  REC_TRY(hipSetDevice(e->device));
  // ---- the blocks the device declined go to zlib: their bytes come back
  e->raw_at.assign(nb, ~0ull);
  uint64_t n_raw = 0, pay = 0;
  for (uint64_t k = 0; k < nb; ++k) { if (bgzf_payload_fits(len[k])) pay += len[k]; else e->raw_at[k] = n_raw++ * BLOCK; }
  if (n_raw) {
    // (dn_pin may move: everything read so far is re-established from the new pointer only when it did not grow -- so the room is asked for up front)
    if (e->dn_pin.cap < a_raw + n_raw * BLOCK + 64) {
      PinBuf more;
      if (!more.need(a_raw + n_raw * BLOCK + 64)) { err = "records_device: out of pinned memory"; return TRGT_ERR_NOMEM; }
      REC_TRY(e->wait());
      std::memcpy(more.p, e->dn_pin.p, a_raw);
      e->dn_pin.release(); e->dn_pin = more;
      P = (uint8_t*)e->dn_pin.p; len = (uint32_t*)(P + a_len);
    }
    for (uint64_t k = 0; k < nb; ++k) if (e->raw_at[k] != ~0ull) REC_TRY(hipMemcpyAsync(P + a_raw + e->raw_at[k], S + k * BLOCK, BLOCK, hipMemcpyDeviceToHost, st));
  }
  REC_TRY(e->wait());
  out.deflated = true; out.payload = P + a_pay; out.len = len; out.crc = (const uint32_t*)(P + a_crc); out.raw = P + a_raw; out.raw_bytes = n_raw * BLOCK; out.raw_at = e->raw_at.data();
  out.tail = P + a_tail; out.tail_bytes = tail_len;
  out.d2h_bytes = nb * 8 + tail_len + pay + n_raw * BLOCK;
  return TRGT_OK;
}

}  // namespace brec
}  // namespace trgt
