// trgt_amd/csrc/hmm.hip -- motif-segmentation HMM on gfx950: log-space Viterbi
// fill, traceback and MS/MC/AP decoding, one allele per workgroup.
//
// Replaces (PacificBiosciences/trgt v3.0.0): build_hmm (src/hmm/builder.rs:4-173),
// Hmm::label (hmm_model.rs:54-156), calc_purity/get_events (purity.rs:6-41,
// events.rs:17-117), remove_imperfect_motifs (operations.rs:6-80), label_motifs
// (hmm_model.rs:158-200), count_motifs/collapse_labels (utils.rs:3-27) as composed
// by label_with_hmm (src/trgt/workflows/tr.rs:454-492).
//
// Kernel shape (see DESIGN.md "K4/K5"): one workgroup per allele, one thread per
// HMM state (workgroup = 64*ceil(S/64) threads; S = 17..26 for one STR motif is a
// single wavefront).  The two live score columns sit in LDS as f64; per base the
// emitting states update in parallel, then the silent states are evaluated level
// by level of their (acyclic) dependency order, so every f64 sum is formed exactly
// as the reference forms it: (prev + ln p) + emission, first strict maximum wins.
// No log() is evaluated on the device: the ln tables come from the host libm.
// Back-pointers are one byte per (base, state), written once to HBM (coalesced
// across the states of a column) and re-read in LDS-staged chunks by the traceback,
// which also classifies events (purity) and collects motif visits on the fly.
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <limits>
#include <thread>

#include "common.hpp"

namespace trgt {

// ------------------------------------------------------------ host model

}  // namespace trgt
#include <memory>

#include "hmm_host.hpp"
namespace trgt {

struct HmmJobDev {
  uint32_t set, seq_len, job_index, path_cap;
  uint64_t seq_off, bp_off, path_off, span_off, count_off, visit_off;
  uint64_t map_off;  // words into the visit workspace: chunk maps of the parallel trace-back of long alleles (0: none, the fill kernel traces back itself)
};

static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Everything about a motif set's model that follows from the motif LENGTHS: number of states, block table (start state, end state,
// motif length, offset of the motif's bytes), the lane -> state table of models of more than one wave, and where the tables sit in the
// set's blob (offsets relative to it).  Shared by the host builder (build_set) and the device builder (hmm_model_build_kernel).
static uint64_t layout_set(const uint32_t* mlen, uint32_t n_motifs, HmmSetDev& d, std::vector<uint32_t>& blocks, std::vector<uint16_t>& perm) {
  uint32_t S = 7, max_mlen = 0, mbytes = 0;
  for (uint32_t i = 0; i < n_motifs; ++i) { S += 3 * mlen[i] + 1; max_mlen = std::max(max_mlen, mlen[i]); }
  const uint32_t nb = n_motifs + 1;
  blocks.assign(4 * (size_t)nb, 0);
  uint32_t ms = 2;
  for (uint32_t mi = 0; mi < n_motifs; ++mi) {
    const uint32_t n = mlen[mi], me = ms + 3 * n;
    blocks[0 * nb + mi] = ms; blocks[1 * nb + mi] = me; blocks[2 * nb + mi] = n; blocks[3 * nb + mi] = mbytes;
    mbytes += n;
    ms = me + 1;
  }
  blocks[0 * nb + nb - 1] = ms; blocks[1 * nb + nb - 1] = ms + 2; blocks[2 * nb + nb - 1] = 0; blocks[3 * nb + nb - 1] = mbytes;  // skip block (builder.rs:41-53)
  // The chain of deletion states of a motif block ends in the block end (d0 .. d0 + n - 2, me = d0 + n - 1: consecutive states, each
  // with the one before it as its LAST predecessor): the kernel walks it across LANES, and a chain that runs over a wave boundary
  // costs it another round.  Models of several waves therefore get a lane -> state table that keeps every chain inside one wave
  // (first fit, longest chain first; the other states fill the lanes left over; a chain longer than a wave starts a wave of its own).
  uint32_t chain_rounds = 1, n_lanes = 0;
  perm.clear();
  if (S > 64) {
    struct Chain { uint32_t first, len; };
    std::vector<Chain> chains;
    std::vector<uint8_t> in_chain(S, 0);
    for (uint32_t b = 0; b + 1 < nb; ++b) {
      const uint32_t n = blocks[2 * nb + b], me = blocks[1 * nb + b];
      if (n > 1) { chains.push_back({me - (n - 1), n}); for (uint32_t s = me - (n - 1); s <= me; ++s) in_chain[s] = 1; }
    }
    std::stable_sort(chains.begin(), chains.end(), [](const Chain& a, const Chain& b) { return a.len > b.len; });
    std::vector<uint32_t> fill;  // lanes used per wave
    auto place = [&](uint32_t lane, uint32_t st) { if (perm.size() <= lane) perm.resize(((size_t)lane / 64 + 1) * 64, 0xFFFF); perm[lane] = (uint16_t)st; };
    for (const Chain& ch : chains) {
      uint32_t w = 0;
      if (ch.len > 64) { w = (uint32_t)fill.size(); }  // whole waves of its own
      else { while (w < fill.size() && fill[w] + ch.len > 64) ++w; }
      const uint32_t waves = (ch.len + 63) / 64;
      if (w + waves > fill.size()) fill.resize(w + waves, 0);
      const uint32_t lane0 = 64 * w + fill[w];
      for (uint32_t k = 0; k < ch.len; ++k) place(lane0 + k, ch.first + k);
      for (uint32_t k = 0; k < waves; ++k) fill[w + k] = k + 1 < waves ? 64 : std::max(fill[w + k], (lane0 + ch.len) - 64 * (w + k));
      chain_rounds = std::max(chain_rounds, (lane0 + ch.len - 1) / 64 - lane0 / 64 + 1);
    }
    uint32_t w = 0;
    for (uint32_t st = 0; st < S; ++st) {
      if (in_chain[st]) continue;
      while (w < fill.size() && fill[w] >= 64) ++w;
      if (w == fill.size()) fill.push_back(0);
      place(64 * w + fill[w], st);
      ++fill[w];
    }
    n_lanes = (uint32_t)perm.size();
  }
  d.S = S; d.n_blocks = nb; d.chain_rounds = chain_rounds; d.max_mlen = max_mlen; d.n_lanes = n_lanes;
  d.ppl_lanes = mbytes + 1 <= 64 ? mbytes + 1 : 0;  // (mbytes = the motif lengths summed up: one lane per motif position, one for the skip block)
  uint64_t o = 0;  // offsets relative to this set's blob; the caller rebases them
  d.off_inlp = o; o += 8ull * 4 * S;
  d.off_em = o; o += 8ull * 5 * S;
  d.off_inst = o; o += 2ull * 4 * S;
  d.off_block = o; o += 2ull * S; o = align_up(o, 4);
  d.off_blocks = o; o += 4ull * 4 * nb;
  d.off_nin = o; o += S;
  d.off_level = o; o += S;
  d.off_flags = o; o += S;
  d.off_motifs = o; o += mbytes; o = align_up(o, 2);
  d.off_perm = o; o += 2ull * perm.size();
  return align_up(o, 16);
}

// build_hmm restated as flat tables (builder.rs:4-173); predecessor ORDER is part of the contract
// because the first strict maximum wins in calc_viterbi_score (hmm_model.rs:79-88).  (Host version: the product builds the tables
// on the device, hmm_model_build_kernel below; this one is what trgt_hmm_models_check compares it with, byte for byte.)
static void build_set(const std::vector<std::string>& motifs, std::vector<uint8_t>& blob, HmmSetDev& d) {
  std::vector<uint32_t> mlens, blocks;
  std::vector<uint16_t> perm;
  for (auto& m : motifs) mlens.push_back((uint32_t)m.size());
  const uint64_t bytes = layout_set(mlens.data(), (uint32_t)mlens.size(), d, blocks, perm);
  const uint32_t S = d.S, nb = d.n_blocks;
  const double NINF = -std::numeric_limits<double>::infinity();
  std::vector<double> inlp(4 * (size_t)S, NINF), em(5 * (size_t)S, NINF);
  std::vector<uint16_t> inst(4 * (size_t)S, 0);
  std::vector<int16_t> block(S, -1);
  std::vector<uint8_t> nin(S, 0), level(S, 0), flags(S, 0);
  std::string mbytes;
  auto set_ems = [&](uint32_t st, const double (&p)[5]) { for (int i = 0; i < 5; ++i) em[(size_t)i * S + st] = std::log(p[i]); };
  auto set_trans = [&](uint32_t st, std::initializer_list<uint32_t> ins, std::initializer_list<double> ps) {
    nin[st] = (uint8_t)ins.size();
    int j = 0;
    for (uint32_t s : ins) inst[(size_t)(j++) * S + st] = (uint16_t)s;
    j = 0;
    for (double p : ps) inlp[(size_t)(j++) * S + st] = std::log(p);
  };
  const double SILENT[5] = {0, 0, 0, 0, 0}, TERM[5] = {1, 0, 0, 0, 0}, UNI[5] = {0.00, 0.25, 0.25, 0.25, 0.25};
  const uint32_t start = 0, end = S - 1, rs = 1, re = S - 2;
  set_ems(start, TERM); set_ems(end, TERM);
  set_trans(end, {re}, {0.10});
  set_ems(rs, SILENT);
  set_trans(rs, {start, re}, {1.00, 1.00});
  const double rs_to_ms = 1.00, me_to_re = 0.50;
  uint32_t ms = rs + 1;
  for (size_t mi = 0; mi < motifs.size(); ++mi) {
    const std::string& motif = motifs[mi];
    const uint32_t n = (uint32_t)motif.size(), me = ms + 3 * n;
    set_ems(ms, SILENT);
    set_trans(ms, {rs, me}, {rs_to_ms, 1.0 - me_to_re});
    // define_motif_block (builder.rs:80-173)
    const uint32_t m0 = ms + 1, i0 = m0 + n, d0 = i0 + n;
    const double match_prob = 0.90, ins_to_ins = 0.25, match_to_indel = (1.00 - match_prob) / 2.00, del_to_match = 0.50;
    const double seed = 2.00 * (1.00 - match_prob) / (double)((size_t)n * (size_t)(n - 1));
    for (uint32_t k = 0; k < n; ++k) {
      double e[5] = {0.00, 0.03, 0.03, 0.03, 0.03};
      switch (motif[k]) {
        case 'A': e[1] = 0.90; break;
        case 'T': e[2] = 0.90; break;
        case 'C': e[3] = 0.90; break;
        case 'G': e[4] = 0.90; break;
        default: e[1] = e[2] = e[3] = e[4] = 0.25; break;  // 'N'
      }
      set_ems(m0 + k, e);
      if (k == 0) set_trans(m0, {ms}, {match_prob});
      else if (k == 1) set_trans(m0 + 1, {m0, ms, i0}, {match_prob, seed * (double)(n - k), 1.0 - ins_to_ins});
      else set_trans(m0 + k, {m0 + k - 1, ms, i0 + k - 1, d0 + k - 2}, {match_prob, seed * (double)(n - k), 1.0 - ins_to_ins, del_to_match});
    }
    for (uint32_t k = 0; k < n; ++k) { set_ems(i0 + k, UNI); set_trans(i0 + k, {i0 + k, m0 + k}, {ins_to_ins, match_to_indel}); }
    for (uint32_t k = 0; k + 1 < n; ++k) {
      set_ems(d0 + k, SILENT);
      if (k == 0) set_trans(d0, {m0}, {match_to_indel});
      else set_trans(d0 + k, {m0 + k, d0 + k - 1}, {match_to_indel, 1.0 - del_to_match});
    }
    set_ems(me, SILENT);
    if (n > 1) set_trans(me, {m0 + n - 1, i0 + n - 1, d0 + n - 2}, {match_prob, 1.0 - ins_to_ins, 1.0});
    else set_trans(me, {m0 + n - 1, i0 + n - 1}, {match_prob, 1.0 - ins_to_ins});
    for (uint32_t s = ms; s <= me; ++s) block[s] = (int16_t)mi;
    mbytes += motif;
    ms = me + 1;
  }
  // skip block (builder.rs:41-53)
  const uint32_t skip = ms + 1, me_skip = ms + 2;
  set_ems(ms, SILENT);
  set_trans(ms, {rs, me_skip}, {rs_to_ms, 1.0 - me_to_re});
  set_ems(skip, UNI);
  set_trans(skip, {ms, skip}, {1.0, 0.5});
  set_ems(me_skip, SILENT);
  set_trans(me_skip, {skip}, {1.0 - 0.5});
  for (uint32_t s = ms; s <= me_skip; ++s) block[s] = (int16_t)(nb - 1);
  // run end: predecessors are the block ends in block order, each ln(me_to_re) (builder.rs:55-57)
  set_ems(re, SILENT);
  nin[re] = 0xFF;
  inlp[re] = std::log(me_to_re);
  // flags; silent states are evaluated after the emitting ones of a column (level 1; any topological order of the silent states
  // gives identical values, hmm_model.rs:206-240 -- the kernel's passes are one)
  for (uint32_t s = 0; s < S; ++s) {
    bool any = false, base = false;
    for (int i = 0; i < 5; ++i) if (std::isfinite(em[(size_t)i * S + s])) { any = true; if (i) base = true; }
    flags[s] = (any ? 1 : 0) | (base ? 2 : 0);
    level[s] = any ? 0 : 1;
  }
  // serialise
  blob.assign((size_t)bytes, 0);
  std::memcpy(&blob[d.off_inlp], inlp.data(), 8ull * 4 * S);
  std::memcpy(&blob[d.off_em], em.data(), 8ull * 5 * S);
  std::memcpy(&blob[d.off_inst], inst.data(), 2ull * 4 * S);
  std::memcpy(&blob[d.off_block], block.data(), 2ull * S);
  std::memcpy(&blob[d.off_blocks], blocks.data(), 4ull * 4 * nb);
  std::memcpy(&blob[d.off_nin], nin.data(), S);
  std::memcpy(&blob[d.off_level], level.data(), S);
  std::memcpy(&blob[d.off_flags], flags.data(), S);
  if (!mbytes.empty()) std::memcpy(&blob[d.off_motifs], mbytes.data(), mbytes.size());
  if (!perm.empty()) std::memcpy(&blob[d.off_perm], perm.data(), 2ull * perm.size());
}

// ---- the same tables built on the device: one workgroup per motif set.  The natural logarithms are the HOST's (the reference's are
// Rust f64::ln = the platform libm, and the scores are sums of them: bit-exact parity needs the very same values): the handful of
// constants comes in by value, ln(seed(n) * (n - k)) from a table with one row per distinct motif length of the batch.
struct HmmBuildConsts {
  double ln_match, ln_1m_ins, ln_del2m, ln_ins2ins, ln_m2indel, ln_1m_del2m, ln_one, ln_1m_me2re, ln_me2re, ln_end, ln_skip_self, ln_skip_out,
         em_hit, em_miss, em_n, em_uni;
};
static HmmBuildConsts hmm_build_consts() {
  const double match_prob = 0.90, ins_to_ins = 0.25, match_to_indel = (1.00 - match_prob) / 2.00, del_to_match = 0.50, me_to_re = 0.50;
  HmmBuildConsts k;
  k.ln_match = std::log(match_prob); k.ln_1m_ins = std::log(1.0 - ins_to_ins); k.ln_del2m = std::log(del_to_match); k.ln_ins2ins = std::log(ins_to_ins);
  k.ln_m2indel = std::log(match_to_indel); k.ln_1m_del2m = std::log(1.0 - del_to_match); k.ln_one = std::log(1.00); k.ln_1m_me2re = std::log(1.0 - me_to_re);
  k.ln_me2re = std::log(me_to_re); k.ln_end = std::log(0.10); k.ln_skip_self = std::log(0.5); k.ln_skip_out = std::log(1.0 - 0.5);
  k.em_hit = std::log(0.90); k.em_miss = std::log(0.03); k.em_n = std::log(0.25); k.em_uni = std::log(0.25);
  return k;
}
struct HmmBuildArgs {
  const HmmSetDev* sets; uint8_t* blob;
  const uint8_t* motif_bytes;       // sanitised motifs of all sets, back to back
  const uint32_t* motif_off;        // [n_motifs_total + 1] into motif_bytes
  const uint32_t* set_motif_begin;  // [n_sets + 1]
  const uint32_t* seed_row;         // [n_motifs_total] first entry of the motif's row of seed_tab (entry k: ln(seed(n) * (n - k)))
  const double* seed_tab;
  const uint16_t* perm_all; const uint64_t* perm_src;  // lane -> state tables of the sets that have one, [n_sets] offsets into perm_all
  uint64_t blob_bytes;              // all sets' tables together (the end of the last set's)
  HmmBuildConsts k;
};
__global__ void __launch_bounds__(64) hmm_model_build_kernel(const HmmBuildArgs a) {
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const HmmSetDev d = a.sets[s];
  const int S = (int)d.S, nb = (int)d.n_blocks;
  const uint32_t mb = a.set_motif_begin[s];
  uint8_t* const blob = a.blob;
  double* inlp = reinterpret_cast<double*>(blob + d.off_inlp);
  double* em = reinterpret_cast<double*>(blob + d.off_em);
  uint16_t* inst = reinterpret_cast<uint16_t*>(blob + d.off_inst);
  int16_t* block = reinterpret_cast<int16_t*>(blob + d.off_block);
  uint32_t* blocks = reinterpret_cast<uint32_t*>(blob + d.off_blocks);
  uint8_t *nin = blob + d.off_nin, *level = blob + d.off_level, *flags = blob + d.off_flags, *mot = blob + d.off_motifs;
  __shared__ uint32_t b_start[256];  // first state of every block (n_blocks <= 254)
  if (tid == 0) {
    uint32_t ms = 2, mbytes = 0;
    for (int mi = 0; mi + 1 < nb; ++mi) {
      const uint32_t n = a.motif_off[mb + mi + 1] - a.motif_off[mb + mi], me = ms + 3 * n;
      blocks[0 * nb + mi] = ms; blocks[1 * nb + mi] = me; blocks[2 * nb + mi] = n; blocks[3 * nb + mi] = mbytes;
      b_start[mi] = ms;
      mbytes += n; ms = me + 1;
    }
    blocks[0 * nb + nb - 1] = ms; blocks[1 * nb + nb - 1] = ms + 2; blocks[2 * nb + nb - 1] = 0; blocks[3 * nb + nb - 1] = mbytes;
    b_start[nb - 1] = ms;
  }
  __syncthreads();
  const double NINF = -__builtin_huge_val();
  const HmmBuildConsts& k = a.k;
  for (int st = tid; st < S; st += 64) {
    double lp[4] = {NINF, NINF, NINF, NINF}, e[5] = {NINF, NINF, NINF, NINF, NINF};
    uint32_t in[4] = {0, 0, 0, 0};
    int n_in = 0, blk = -1;
    if (st == 0) { e[0] = k.ln_one; }                                                   // start: emits '#'
    else if (st == S - 1) { e[0] = k.ln_one; n_in = 1; in[0] = (uint32_t)S - 2; lp[0] = k.ln_end; }   // end <- run end
    else if (st == 1) { n_in = 2; in[0] = 0; in[1] = (uint32_t)S - 2; lp[0] = k.ln_one; lp[1] = k.ln_one; }  // run start <- {start, run end}
    else if (st == S - 2) { n_in = 0xFF; lp[0] = k.ln_me2re; }                          // run end <- the block ends
    else {
      int lo = 0, hi = nb - 1;  // the block of the state
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (b_start[mid] <= (uint32_t)st) lo = mid; else hi = mid - 1; }
      blk = lo;
      const uint32_t ms = b_start[blk];
      if (blk == nb - 1) {  // skip block
        const uint32_t skip = ms + 1, me = ms + 2;
        if ((uint32_t)st == ms) { n_in = 2; in[0] = 1; in[1] = me; lp[0] = k.ln_one; lp[1] = k.ln_1m_me2re; }
        else if ((uint32_t)st == skip) { e[1] = e[2] = e[3] = e[4] = k.em_uni; n_in = 2; in[0] = ms; in[1] = skip; lp[0] = k.ln_one; lp[1] = k.ln_skip_self; }
        else { n_in = 1; in[0] = skip; lp[0] = k.ln_skip_out; }
      } else {
        const uint32_t mo = a.motif_off[mb + blk], n = a.motif_off[mb + blk + 1] - mo;
        const uint32_t me = ms + 3 * n, m0 = ms + 1, i0 = m0 + n, d0 = i0 + n;
        const double* seed = a.seed_tab + a.seed_row[mb + blk];
        if ((uint32_t)st == ms) { n_in = 2; in[0] = 1; in[1] = me; lp[0] = k.ln_one; lp[1] = k.ln_1m_me2re; }
        else if ((uint32_t)st == me) {
          if (n > 1) { n_in = 3; in[0] = m0 + n - 1; in[1] = i0 + n - 1; in[2] = d0 + n - 2; lp[0] = k.ln_match; lp[1] = k.ln_1m_ins; lp[2] = k.ln_one; }
          else { n_in = 2; in[0] = m0 + n - 1; in[1] = i0 + n - 1; lp[0] = k.ln_match; lp[1] = k.ln_1m_ins; }
        } else if ((uint32_t)st < i0) {  // match state
          const uint32_t kk = (uint32_t)st - m0;
          const uint8_t c = a.motif_bytes[mo + kk];
          if (c == 'A' || c == 'T' || c == 'C' || c == 'G') { e[1] = e[2] = e[3] = e[4] = k.em_miss; e[c == 'A' ? 1 : c == 'T' ? 2 : c == 'C' ? 3 : 4] = k.em_hit; }
          else e[1] = e[2] = e[3] = e[4] = k.em_n;
          if (kk == 0) { n_in = 1; in[0] = ms; lp[0] = k.ln_match; }
          else if (kk == 1) { n_in = 3; in[0] = m0; in[1] = ms; in[2] = i0; lp[0] = k.ln_match; lp[1] = seed[1]; lp[2] = k.ln_1m_ins; }
          else { n_in = 4; in[0] = m0 + kk - 1; in[1] = ms; in[2] = i0 + kk - 1; in[3] = d0 + kk - 2; lp[0] = k.ln_match; lp[1] = seed[kk]; lp[2] = k.ln_1m_ins; lp[3] = k.ln_del2m; }
        } else if ((uint32_t)st < d0) {  // insertion state
          const uint32_t kk = (uint32_t)st - i0;
          e[1] = e[2] = e[3] = e[4] = k.em_uni;
          n_in = 2; in[0] = i0 + kk; in[1] = m0 + kk; lp[0] = k.ln_ins2ins; lp[1] = k.ln_m2indel;
        } else {  // deletion state
          const uint32_t kk = (uint32_t)st - d0;
          if (kk == 0) { n_in = 1; in[0] = m0; lp[0] = k.ln_m2indel; }
          else { n_in = 2; in[0] = m0 + kk; in[1] = d0 + kk - 1; lp[0] = k.ln_m2indel; lp[1] = k.ln_1m_del2m; }
        }
      }
    }
    bool any = false, base = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) { em[(size_t)i * S + st] = e[i]; if (e[i] > NINF) { any = true; if (i) base = true; } }
#pragma unroll
    for (int j = 0; j < 4; ++j) { inlp[(size_t)j * S + st] = lp[j]; inst[(size_t)j * S + st] = (uint16_t)in[j]; }
    block[st] = (int16_t)blk; nin[st] = (uint8_t)n_in; flags[st] = (uint8_t)((any ? 1 : 0) | (base ? 2 : 0)); level[st] = any ? 0 : 1;
  }
  {  // motif bytes, lane table, padding
    const uint32_t m_lo = a.motif_off[mb], m_hi = a.motif_off[mb + nb - 1];
    if (tid == 0) {  // the alignment gaps of the set's tables (layout_set): zero, as in the host builder's blob
      const uint64_t end = (uint32_t)s + 1u < gridDim.x ? a.sets[s + 1].off_inlp : a.blob_bytes;
      for (uint64_t q = d.off_block + 2ull * (uint64_t)S; q < d.off_blocks; ++q) blob[q] = 0;
      for (uint64_t q = d.off_motifs + (uint64_t)(m_hi - m_lo); q < d.off_perm; ++q) blob[q] = 0;
      for (uint64_t q = d.off_perm + 2ull * d.n_lanes; q < end; ++q) blob[q] = 0;
    }
    for (uint32_t i = (uint32_t)tid; i < m_hi - m_lo; i += 64) mot[i] = a.motif_bytes[m_lo + i];
    if (d.n_lanes) {
      uint16_t* perm = reinterpret_cast<uint16_t*>(blob + d.off_perm);
      const uint16_t* src = a.perm_all + a.perm_src[s];
      for (uint32_t i = (uint32_t)tid; i < d.n_lanes; i += 64) perm[i] = src[i];
    }
  }
}

// --------------------------------------------------------------- kernel
#ifdef TRGT_HMM_PROF
// developer build (make HMMPROF=1): lane 0 of every job splits its shader-clock time over the phases of the kernel
__device__ unsigned long long g_hmm_prof[16];
#define HP_DECL unsigned long long hp_t = clock64()
#define HP_MARK(i) do { const unsigned long long n_ = clock64(); if (tid == 0) atomicAdd(&g_hmm_prof[i], n_ - hp_t); hp_t = n_; } while (0)
#define HP_FILL_DECL unsigned long long hf_t = clock64(), hf_acc[6] = {0, 0, 0, 0, 0, 0}
#define HP_FILL(i) do { const unsigned long long n_ = clock64(); hf_acc[i] += n_ - hf_t; hf_t = n_; } while (0)
#define HP_FILL_END do { if (tid == 0) for (int q_ = 0; q_ < 6; ++q_) atomicAdd(&g_hmm_prof[8 + q_], hf_acc[q_]); } while (0)
#define HP_LONG_DECL unsigned long long hl_t = clock64()
#define HP_LONG(i) do { const unsigned long long n_ = clock64(); if (tid == 0) atomicAdd(&g_hmm_prof[i], n_ - hl_t); hl_t = n_; } while (0)
#else
#define HP_DECL
#define HP_MARK(i)
#define HP_FILL_DECL
#define HP_FILL(i)
#define HP_FILL_END
#define HP_LONG_DECL
#define HP_LONG(i)
#endif
constexpr int HMM_LONG_MIN = 1536;   // columns from which an allele's trace-back goes to hmm_traceback_long_kernel (round 5, tried 512: the cfg3 call 9.5 -> 9.3 ms, but the hundreds of 0.5-2 kb VNTR alleles of a cfg4 step through the many-wave kernel 9.1 -> 11.5 ms)
constexpr int HMM_LONG_CHUNK = 64;   // columns per chunk map there
constexpr int HMM_STAGE_BYTES = 1024;  // LDS staging window for back-pointer columns during traceback (one-wave models)
// ... models of several waves (rows of 80 to 320 bytes) stage 16 columns at a time: 1 KB held five columns of a 192-state model, and every
// chunk costs a global round trip and two barriers
__host__ __device__ constexpr int hmm_stage_bytes(int spad) { return spad > 64 ? (16 * spad > HMM_STAGE_BYTES ? 16 * spad : HMM_STAGE_BYTES) : HMM_STAGE_BYTES; }
constexpr int HMM_LDS_PER_STATE = 16 + 16 + 40 + 4 + 16 + 2 + 1 + 1;  // two score columns, lp[2], em[5], info, inst[4] (32-bit entries), block, flags, bp column

__device__ __forceinline__ int hmm_code(const uint8_t* __restrict__ seq, int i, int L) {
  // '#'+seq+'#' with encode_base (hmm_model.rs:243-252) after replace_invalid_bases(seq, ATCG) (utils.rs:29-42)
  if (i == 0 || i == L - 1) return 0;
  const uint8_t b = seq[i - 1];
  return b == 'A' ? 1 : b == 'T' ? 2 : b == 'C' ? 3 : b == 'G' ? 4 : ((i - 1) & 3) + 1;
}

// "#ATCG"[code] without a memory access (a string constant is a global load: a round trip per trace-back step)
__device__ __forceinline__ int hmm_code_char(int code) { return (int)((0x4743544123ull >> (8 * code)) & 0xFFull); }

// Workgroup synchronisation of the Viterbi kernel.  Most motif sets need at most 64 states, i.e. a single wavefront: its lanes run in
// lockstep and the LDS unit serves one wave's accesses in order, so a compiler-level fence is all that is needed -- whereas
// __syncthreads() also waits for every global store in flight (the back-pointer column written at the end of each step), a
// memory round trip per step.
// Several waves: an LDS-only barrier.  __syncthreads() is s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier, and the vmcnt(0) makes every
// one of the four barriers of a column wait for the back-pointer stores of the column before (a round trip to L2 each, most of a
// column's time for the 170- to 190-state models); those bytes are read again only by the trace-back, behind hmm_sync_mem().
__device__ __forceinline__ void hmm_sync(int nthr) {
  if (nthr == 64) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// ... and the full one: global stores of the whole workgroup are visible afterwards
__device__ __forceinline__ void hmm_sync_mem(int nthr) {
  if (nthr == 64) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  else __syncthreads();
}

// LDS of a job does not depend on the length of its allele (it bounds the waves per SIMD of a kernel that is bound by instruction
// issue and dependent LDS round trips): the fill and the trace-back see the allele through a WINDOW of symbol codes, the trace-back
// keeps the first HMM_VIS_LDS motif visits in LDS and the rest in the job's global workspace (read back in staged chunks), the
// check of the motif copies (remove_imperfect_motifs) happens in the trace-back, where the window holds their bases.
constexpr int HMM_CODE_WINDOW = 256;  // columns of symbol codes kept in LDS (+ HMM_CODE_PAD behind them)
constexpr int HMM_CODE_PAD = 16;      // the column after the window (fill), the bases of a motif copy that starts at its end (trace-back)
constexpr int HMM_VIS_LDS = 64;       // motif visits kept in LDS (block | dropped << 15, first base, one past the last base)
// SUB: lanes per allele.  64 (or more: one thread per state, several waves for large motif sets) is the general case; SUB = 32
// packs TWO alleles into one wave when the model has at most 32 states (a single STR motif of up to 8 bases): the kernel is bound
// by instruction issue and most passes of a column keep only one or two lanes busy, so halving the waves nearly halves its time.
// The two halves run the same code on their own LDS regions; their control flow may diverge (different allele lengths).
// the value of the lane before (lane 0: its own)
__device__ __forceinline__ double wave_shr1_f64(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const int lo = (int)(u & 0xFFFFFFFFull), hi = (int)(u >> 32);
  const int slo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xF, 0xF, false);  // wave_shr:1
  const int shi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)shi << 32) | (unsigned)slo));
}

// max of two scores: the value of (a > b ? a : b) -- scores are never NaN or -0.0 -- in ONE v_max_f64 (fmax() comes with a canonicalising
// v_max_f64 x, x in front of it: 16 more cycles in a loop that runs once per base of the longest motif per column)
__device__ __forceinline__ double max_f64(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// f64 from another lane of the wave (byte address of the source lane: lane << 2)
__device__ __forceinline__ double bperm_f64(int addr, double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const int lo = __builtin_amdgcn_ds_bpermute(addr, (int)(u & 0xFFFFFFFFull)), hi = __builtin_amdgcn_ds_bpermute(addr, (int)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// ---- the packed back-pointer rows of hmm_fill_ppl_kernel<G, true> (hmm_ppl.hpp): one byte per LANE (motif position) and column.
__host__ __device__ inline int hmm_ppl_group(uint32_t positions) { return positions == 0 || positions > 64 ? 0 : positions <= 8 ? 8 : positions <= 16 ? 16 : positions <= 32 ? 32 : 64; }
// Where the back-pointer of state `st` lies in such a row: lane | shift << 6 | mask << 9 (mask 0: a state whose back-pointer is a constant 0 --
// the end state -- or is never read; the run end's block index is spread over the lanes 1-3: hmm_bp_run_end).  blocks: [4][nb] start state,
// end state, motif length, first position (= lane) of every block; blk: the state's block (-1: outside the blocks).
__device__ __forceinline__ uint32_t hmm_bp_loc(int st, int nb, int blk, const uint32_t* blocks) {
  if (st == 1) return 0u | (6u << 6) | (3u << 9);               // run start: lane 0, bits 6-7
  if (blk < 0) return 0u;
  const int ms = (int)blocks[blk], n = (int)blocks[2 * nb + blk], off = st - ms;
  const uint32_t pos0 = blocks[3 * nb + blk];
  if (off == 0) return pos0 | (5u << 6) | (1u << 9);            // block start: bit 5 of the block's first lane
  if (blk == nb - 1) return off == 1 ? (pos0 | (0u << 6) | (3u << 9)) : (pos0 | (3u << 6) | (3u << 9));  // skip state | skip block's end
  if (off <= n) return (pos0 + (uint32_t)(off - 1)) | (0u << 6) | (3u << 9);              // match state k
  if (off <= 2 * n) return (pos0 + (uint32_t)(off - n - 1)) | (2u << 6) | (1u << 9);      // insertion state k
  return (pos0 + (uint32_t)(off - 2 * n - 1)) | (3u << 6) | (3u << 9);                    // deletion state k / block end (k = n - 1)
}
__device__ __forceinline__ uint32_t hmm_bp_unpack(uint32_t byte, uint32_t loc) { return (byte >> ((loc >> 6) & 7u)) & (loc >> 9); }
__device__ __forceinline__ uint32_t hmm_bp_run_end(uint32_t row_word) { return ((row_word >> 14) & 3u) | ((row_word >> 20) & 0xCu) | ((row_word >> 26) & 0x30u); }
// loc of the end state of block b (the deletion slot of its last position; the skip block has one position)
__device__ __forceinline__ uint32_t hmm_bp_loc_block_end(int b, int nb, const uint32_t* blocks) {
  const uint32_t n = blocks[2 * nb + b];
  return (blocks[3 * nb + b] + (n ? n - 1u : 0u)) | (3u << 6) | (3u << 9);
}
// predecessor entries of the trace-backs: predecessor state | its "emits" bit << 15 | its hmm_bp_loc << 16 (what the chase needs to know
// about a state is there when it arrives in it: one LDS round trip per step)
__device__ __forceinline__ uint32_t hmm_pred_entry(uint32_t pr, int S, int nb, const uint8_t* g_flags, const int16_t* g_block, const uint32_t* g_blocks) {
  if (pr >= (uint32_t)S) return pr;
  return pr | ((uint32_t)(g_flags[pr] & 1) << 15) | (hmm_bp_loc((int)pr, nb, (int)g_block[pr], g_blocks) << 16);
}

#include "hmm_traceback.hpp"

// ONE_WAVE (models of at most 64 states: one state per lane of ONE wave, or two alleles of at most 32 states in its halves): the score
// columns of the fill live in REGISTERS -- a state's predecessors are fetched from their lanes (ds_bpermute: one LDS-crossbar round per
// pass, nothing written) instead of through two LDS arrays (a write, a fence and a read per pass), and what the run-end lane worked out
// alone (the maximum over the block ends, the run start behind it) every lane of the job works out for itself from the same fetched
// values.  Same sums, same predecessor order, same strict '>'.
template <int SUB, bool ONE_WAVE>
__global__ void hmm_viterbi_kernel(const HmmJobDev* __restrict__ jobs, const HmmSetDev* __restrict__ sets,
                                   const uint8_t* __restrict__ model, const uint8_t* __restrict__ seq_blob,
                                   uint8_t* __restrict__ bp_ws, uint32_t* __restrict__ visit_ws,
                                   uint16_t* __restrict__ path, uint32_t* __restrict__ path_len,
                                   int32_t* __restrict__ spans3, uint32_t* __restrict__ n_spans,
                                   uint32_t* __restrict__ counts, double* __restrict__ purity,
                                   int32_t* __restrict__ edit_out, int32_t* __restrict__ maxd_out,
                                   uint32_t n_launch_jobs, uint32_t lds_per_job, const uint32_t* __restrict__ n_jobs_dev, uint32_t* __restrict__ long_list) {
  extern __shared__ __align__(16) unsigned char lds_all[];
  if (n_jobs_dev) n_launch_jobs = *n_jobs_dev;  // a job list resolved on the device (hmm_resolve_kernel): the grid covers all candidates
  const bool four_rounds = (lds_per_job >> 31) != 0u;  // (TRGT_HMM_FOUR_ROUNDS, see the register fill)
  const bool ppl_filled = ((lds_per_job >> 30) & 1u) != 0u;
  const bool ppl_packed = ((lds_per_job >> 23) & 1u) != 0u;  // ... in rows of one byte per lane (hmm_fill_ppl_kernel<G, true>)
  const int long_min = ((lds_per_job >> 24) & 0x3Fu) ? (int)((lds_per_job >> 24) & 0x3Fu) * 256 : HMM_LONG_MIN;  // (by the size of the class, hmm_long_min)  // the back-pointers of sets with ppl_lanes are there already (hmm_fill_ppl_kernel ran in front)
  lds_per_job &= 0x007FFFFFu;
  const int grp = SUB == 32 ? (int)(threadIdx.x >> 5) : 0;
  const int tid = SUB == 32 ? (int)(threadIdx.x & 31) : (int)threadIdx.x, nthr = SUB == 32 ? 32 : (int)blockDim.x;
  const int sync_n = SUB == 32 ? 64 : (int)blockDim.x;  // see hmm_sync: a single wave needs no barrier
  const uint32_t jidx = SUB == 32 ? blockIdx.x * 2u + (uint32_t)grp : blockIdx.x;
  if (jidx >= n_launch_jobs) return;
  HP_DECL;
  unsigned char* const lds = lds_all + (size_t)grp * lds_per_job;
  const HmmJobDev job = jobs[jidx];
  const HmmSetDev set = sets[job.set];
  const int S = (int)set.S, nb = (int)set.n_blocks, n_motifs = nb - 1;
  const int qlen = (int)job.seq_len, L = qlen + 2;
  const int Spad = (S + 15) & ~15;
  const double NINF = -__builtin_huge_val();

  for (int m = tid; m < n_motifs; m += nthr) counts[job.count_off + m] = 0;
  if (qlen == 0) {  // Hmm::label returns an empty path; calc_purity returns NaN (hmm_model.rs:145-147, purity.rs:7-9)
    if (tid == 0) {
      if (path_len) path_len[job.job_index] = 0;
      n_spans[job.job_index] = 0;
      purity[job.job_index] = __builtin_nan("");
      if (edit_out) edit_out[job.job_index] = 0;
      if (maxd_out) maxd_out[job.job_index] = 0;
    }
    return;
  }
  // ---- LDS carve-up (all dynamic, 16-byte aligned pieces; no static LDS in front of it)
  int* tb = reinterpret_cast<int*>(lds);  // traceback state shared between the walker and the stagers
  uint32_t* l_inst = reinterpret_cast<uint32_t*>(lds + 64);           // [S][4] hmm_pred_entry (predecessor b of state s at 4 s + b: 16 bytes per state, one read)
  double* sc0 = reinterpret_cast<double*>(l_inst + 4 * S);
  double* sc1 = sc0 + S;
  double* l_lp = sc1 + S;                                             // [2][S] ln transition probabilities of predecessors 0 and 1
  double* l_em = l_lp + 2 * S;                                        // [5][S] ln emission probabilities by symbol code: one LDS read per column instead of a select tree
  uint32_t* l_info = reinterpret_cast<uint32_t*>(l_em + 5 * S);       // [S] what the traceback needs to know about a state, in one word
  int16_t* l_block = reinterpret_cast<int16_t*>(l_info + S);         // [S]
  uint8_t* l_flags = reinterpret_cast<uint8_t*>(l_block + S);        // [S]
  uint8_t* l_bpcol = l_flags + S;                                     // [S] back-pointers of states evaluated by another lane
  uint32_t* l_blocks = reinterpret_cast<uint32_t*>(lds + 64 + (((size_t)HMM_LDS_PER_STATE * S + 15) & ~(size_t)15));  // [4][nb]
  uint8_t* l_stage = lds + 64 + (((size_t)HMM_LDS_PER_STATE * S + 15) & ~(size_t)15) + (((size_t)16 * nb + 15) & ~(size_t)15);

  const double* g_inlp = reinterpret_cast<const double*>(model + set.off_inlp);
  const double* g_em = reinterpret_cast<const double*>(model + set.off_em);
  const uint16_t* g_inst = reinterpret_cast<const uint16_t*>(model + set.off_inst);
  const int16_t* g_block = reinterpret_cast<const int16_t*>(model + set.off_block);
  const uint32_t* g_blocks = reinterpret_cast<const uint32_t*>(model + set.off_blocks);
  const uint8_t* g_motifs = model + set.off_motifs;
  // behind the back-pointer staging window: window of symbol codes | motif bytes | motif visits | motif counts
  uint8_t* l_seq = l_stage + hmm_stage_bytes(Spad);
  uint8_t* l_mot = l_seq + HMM_CODE_WINDOW + HMM_CODE_PAD;
  const int mot_bytes = (S - 7 - n_motifs) / 3;
  uint32_t* l_vis = reinterpret_cast<uint32_t*>(l_mot + ((mot_bytes + 15) & ~15));
  uint32_t* l_cnt = l_vis + 3 * HMM_VIS_LDS;
  uint32_t* l_rec = l_cnt + ((nb + 1) & ~1);  // [HMM_REC_MAX][2] (state, column) of the steps of a trace-back round
  for (int i = tid; i < mot_bytes; i += nthr) l_mot[i] = g_motifs[i];
  for (int i = tid; i < n_motifs; i += nthr) l_cnt[i] = 0;
  const uint8_t* const motif_bytes = l_mot;
  // (bit 15 of a predecessor entry: that state emits a base -- the trace-back then knows it on arrival, without a look-up of its own)
  for (int i = tid; i < 4 * S; i += nthr) l_inst[4 * (i % S) + i / S] = hmm_pred_entry(g_inst[i], S, nb, model + set.off_flags, g_block, g_blocks);
  // (a job whose back-pointers the position-per-lane fill has written is only traced back here: the transition / emission tables and the
  //  per-state registers of this kernel's own fill are not loaded for it -- a dozen rounds of global loads per job)
  const bool own_fill = !(ppl_filled && set.ppl_lanes != 0u);
  for (int i = tid; i < S; i += nthr) { l_block[i] = g_block[i]; l_flags[i] = model[set.off_flags + i]; if (own_fill) { l_lp[i] = g_inlp[i]; l_lp[S + i] = g_inlp[S + i]; } }
  if (own_fill) for (int i = tid; i < 5 * S; i += nthr) l_em[i] = g_em[i];
  for (int i = tid; i < 4 * nb; i += nthr) l_blocks[i] = g_blocks[i];

  // ---- my state's tables in registers
  // (models of several waves: the lane -> state table of build_set, which keeps every deletion chain inside one wave)
  const int st_lane = set.n_lanes ? (int)reinterpret_cast<const uint16_t*>(model + set.off_perm)[tid] : tid;
  const bool act = st_lane < S;
  const int st = act ? st_lane : 0;
  const int n_in = own_fill ? (int)model[set.off_nin + st] : 0;
  const int level = own_fill ? (int)model[set.off_level + st] : 0;
  double lp0 = 0.0, lp1 = 0.0, lp2 = 0.0, lp3 = 0.0;
  int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  if (own_fill) {
    lp0 = g_inlp[0 * S + st]; lp1 = g_inlp[1 * S + st]; lp2 = g_inlp[2 * S + st]; lp3 = g_inlp[3 * S + st];
    p0 = g_inst[0 * S + st]; p1 = g_inst[1 * S + st]; p2 = g_inst[2 * S + st]; p3 = g_inst[3 * S + st];
  }
  // predecessor slots that do not exist read score 0 of state 0 and are ignored (n_in guards the comparison)
  const int q0 = (n_in != 0xFF && n_in > 0) ? p0 : 0, q1 = (n_in != 0xFF && n_in > 1) ? p1 : 0, q2 = (n_in != 0xFF && n_in > 2) ? p2 : 0, q3 = (n_in != 0xFF && n_in > 3) ? p3 : 0;
  const uint8_t* __restrict__ seq = seq_blob + job.seq_off;
  // Symbol code of column i ('#' + allele + '#', hmm_code): from the window l_seq, columns [win0, win0 + HMM_CODE_WINDOW + pad).  A
  // load per column from global memory put a memory round trip -- and, the loads and the back-pointer stores sharing one in-order
  // counter, the store of the column before -- into every step.
  int win0 = 0;
  auto code_at = [&](int i) -> int { return (int)l_seq[i - win0]; };
  uint8_t* __restrict__ bp = bp_ws + job.bp_off;
  hmm_sync_mem(sync_n);  // (also orders the zeroing of the motif counts above before thread 0 counts into them)
  // traceback word of my state: kind (0 outside any block, 1 block start, 2 block end, 3 skip state, 4 match, 5 insertion,
  // 6 deletion) | emits << 3 | block << 8 | expected motif base << 16 (match states)
  if (act) l_info[st] = hmm_state_info(st, (int)l_block[st], nb, l_blocks, motif_bytes, l_flags[st]);
  // roles in the evaluation of the silent states of a column (see the fill loop)
  const int my_blk = act ? (int)l_block[st] : -1;
  const bool role_end = act && my_blk >= 0 && st == (int)l_blocks[1 * nb + my_blk];
  const bool role_start = act && my_blk >= 0 && st == (int)l_blocks[0 * nb + my_blk];
  const bool role_del = act && level > 0 && !role_end && !role_start && n_in != 0xFF && my_blk >= 0;  // deletion states
  const bool role_chain = role_del || role_end;
  // a chain state's LAST predecessor is the state before it (deletion state k: {match k, deletion k - 1}; block end: {last match,
  // last insertion, last deletion}) -- the lane before it, or the last lane of the wave before
  const bool chain_prev = role_del ? n_in > 1 : role_end ? n_in > 2 : false;
  const bool chain_xwave = chain_prev && (threadIdx.x & 63u) == 0;
  // (every lane runs the chain steps: -inf as the transition term of the lanes that take nothing from their neighbour -- and of the
  //  first lane of a wave, which takes its predecessor from LDS before the steps -- makes their candidate lose every comparison)
  const double lp_chain = role_del ? lp1 : lp2, lp_step = chain_prev && !chain_xwave ? lp_chain : NINF;
  const int chain_steps = __builtin_amdgcn_readfirstlane(min(63, max((int)set.max_mlen, SUB == 32 ? __shfl_xor((int)set.max_mlen, 32) : 0) - 1));  // (the same in every lane: a scalar loop count)
  const int chain_rounds = (int)set.chain_rounds;
  // (waves of a multi-wave model that hold no chain state skip the steps: they only cost issue slots of their SIMD)
  const bool wave_chain = __ballot(lp_step > NINF) != 0ull;

  HP_MARK(0);
  // the run-end state's predecessors (the block ends, in block order): the first BE_REG of them by index in registers
  const double lp_rs0 = l_lp[1], lp_rs1 = l_lp[S + 1];  // transition terms of the run start (state 1), evaluated by the run-end lane
  constexpr int BE_REG = 8;
  int be[BE_REG];
#pragma unroll
  for (int b = 0; b < BE_REG; ++b) be[b] = (int)l_blocks[1 * nb + (b < nb ? b : 0)];
  // ---- Viterbi fill (generate_mats, hmm_model.rs:99-114)
  // Two rounds of cross-lane traffic per column instead of four (register fill: crossbar fetches; LDS fill: barriers).  What the silent states of a column need is final early: the deletion chains
  // and block ends after the chain pass, and run end / run start / block starts are then plain functions of THOSE -- every lane
  // works them out for itself from one round of fetches (block ends, start state, its own block's end): the run end as before, the
  // run start behind it, and the start of its own block {run start, own block end}.  The same round fetches the predecessors of
  // the NEXT column's emitting states (emitting, deletion and block-end states: final by then); a predecessor that is a block
  // start or the run end is taken from the lane's own copy.  Same sums, same order, same strict '>'.  The topology this rests on
  // (builder.rs:4-173) is checked per job: block start = {run start, own block end}; an emitting state's silent predecessors are
  // deletion states, block ends, its OWN block's start (slot 0 or 1) or the run end (slot 0) -- anything else takes the loop
  // with one round per pass below.
  const int my_ms = my_blk >= 0 ? (int)l_blocks[0 * nb + my_blk] : 0, my_me = my_blk >= 0 ? (int)l_blocks[1 * nb + my_blk] : 0;
  const double ms_lp0 = my_blk >= 0 ? l_lp[my_ms] : NINF, ms_lp1 = my_blk >= 0 ? l_lp[S + my_ms] : NINF;
  bool bad = false, use_loc0 = false, use_loc1 = false;
  if (own_fill && act && my_blk >= 0) bad = model[set.off_nin + my_ms] != 2 || g_inst[0 * S + my_ms] != 1 || g_inst[1 * S + my_ms] != my_me;
  if (own_fill && act && level == 0 && n_in != 0xFF) {
    for (int b = 0; b < n_in && b < 4; ++b) {
      const int pb = b == 0 ? p0 : b == 1 ? p1 : b == 2 ? p2 : p3;
      const int pblk = pb < S ? (int)l_block[pb] : -1;
      const bool p_start = pblk >= 0 && pb == (int)l_blocks[0 * nb + pblk];
      if (pb == 1) bad = true;                                   // the run start feeds block starts only
      else if (pb == S - 2) { if (b == 0) use_loc0 = true; else bad = true; }
      else if (p_start) {
        if (pblk == my_blk && b == 0) use_loc0 = true;
        else if (pblk == my_blk && b == 1) use_loc1 = true;
        else bad = true;
      }
    }
  }
  const bool two_rounds = !(sync_n == 64 ? __ballot(bad) != 0ull : __syncthreads_or(bad ? 1 : 0) != 0) && !four_rounds;
  double* prev = sc0;
  double* cur = sc1;
  HP_FILL_DECL;
  int sym_next = 0;
  if (own_fill) {
  if constexpr (ONE_WAVE) {
    const int hw = (int)(threadIdx.x & 63u), lane_base = hw & ~(SUB - 1);
    const int a_q0 = (lane_base + q0) << 2, a_q1 = (lane_base + q1) << 2, a_q2 = (lane_base + q2) << 2, a_q3 = (lane_base + q3) << 2, a_st0 = lane_base << 2;
    int a_be[BE_REG];
#pragma unroll
    for (int b = 0; b < BE_REG; ++b) a_be[b] = (lane_base + be[b]) << 2;
    const double lp_re = l_lp[S - 2];  // the run end's transition term (one for all its predecessors' slot 0 ... see below)
    const int a_myend = (lane_base + my_me) << 2;
    const bool is_run_end = act && n_in == 0xFF, is_run_start = act && st == 1;
    if (two_rounds) {
      // (What a column costs the one wave is issue slots: a ds_bpermute_b32 of a permutation ~32 cycles, 14 when all lanes read one
      //  lane, an f64 add or compare ~16, tools/micro/bperm_cost.hip.  Tried on top of this loop and dropped, each slower or even:
      //  block ends by v_readlane, predecessor 0 by a DPP shift, the own block end picked from the block ends (each also on its own:
      //  6.0 -> 6.5 / 6.25 ms for a class of a cfg3 call), every "first maximum" as a tournament with -inf transition terms in the
      //  invalid slots -- fewer crossbar passes, more selects and uniform branches that split the column's one basic block.)
      double em_next = 0.0;
      const bool loc_is_re = act && use_loc0 && p0 == S - 2;
      double pe0 = NINF, pe1 = NINF, pe2 = NINF, pe3 = NINF;  // the predecessors' scores of the column before
      uint8_t* __restrict__ bp_col = bp;
      // (column 0 is a copy of its own: the start state's special case and the run start's first candidate cost no branch per column)
      auto column = [&](const int i, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        // (symbol codes two columns ahead, emission terms one: neither LDS round trip is waited for in the column that starts it)
        if ((i % HMM_CODE_WINDOW) == 0) {
          hmm_sync(sync_n);
          win0 = i;
          for (int k = tid; k < HMM_CODE_WINDOW + 2 && i + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, i + k, L);
          hmm_sync(sync_n);
          sym_next = code_at(i);
          em_next = l_em[sym_next * S + st];
          sym_next = i + 1 < L ? code_at(i + 1) : 0;
        }
        const double em = em_next;
        em_next = l_em[__umul24((unsigned)sym_next, (unsigned)S) + st];
        sym_next = i + 2 < L ? code_at(i + 2) : 0;
        HP_FILL(0);
        double best = NINF;
        int bpi = 0xFF;
        if (act && level == 0) {
          if constexpr (FIRST) {
            if (n_in == 0 && em > NINF) { best = em; bpi = 0xFE; }  // the start state (hmm_model.rs:91-94)
          } else {
            const double v0 = (pe0 + lp0) + em, v1 = (pe1 + lp1) + em, v2 = (pe2 + lp2) + em, v3 = (pe3 + lp3) + em;
            if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
            if (n_in > 1 && v1 > best) { best = v1; bpi = 1; }
            if (n_in > 2 && v2 > best) { best = v2; bpi = 2; }
            if (n_in > 3 && v3 > best) { best = v3; bpi = 3; }
          }
        }
        double cur_v = best;
        HP_FILL(1);
        {  // round 1: the chains d0 <- d1 <- ... <- block end take this column's emitting states
          const double s0 = bperm_f64(a_q0, cur_v), s1 = bperm_f64(a_q1, cur_v);
          if (role_chain) {
            const double v0 = (s0 + lp0), v1 = (s1 + lp1);
            if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
            if (role_end && n_in > 1 && v1 > best) { best = v1; bpi = 1; }
          }
          double val = best, cand = NINF;
          for (int t = 0; wave_chain && t < chain_steps; ++t) {
            cand = (wave_shr1_f64(val) + lp_step);
            val = max_f64(cand, best);
          }
          if (cand > best) bpi = role_del ? 1 : 2;
          best = val;
          if (role_chain) cur_v = val;
        }
        HP_FILL(2);
        {  // round 2: block ends, start state, own block end -- and the next column's predecessors
          const double f0 = bperm_f64(a_q0, cur_v), f1 = bperm_f64(a_q1, cur_v), f2 = bperm_f64(a_q2, cur_v), f3 = bperm_f64(a_q3, cur_v);
          const double myend = bperm_f64(a_myend, cur_v);
          double re = NINF; int re_bp = 0xFF;
          auto block_ends = [&](auto n_const) {
            constexpr int N = decltype(n_const)::value;
            double e[N];
#pragma unroll
            for (int b = 0; b < N; ++b) e[b] = bperm_f64(a_be[b], cur_v);
#pragma unroll
            for (int b = 0; b < N; ++b) {
              const double v = (e[b] + lp_re);
              if (b < nb && v > re) { re = v; re_bp = b; }
            }
          };
          if (nb <= 2) block_ends(std::integral_constant<int, 2>());
          else if (nb <= 4) block_ends(std::integral_constant<int, 4>());
          else block_ends(std::integral_constant<int, BE_REG>());
          for (int b = BE_REG; b < nb; ++b) {
            const double v = (bperm_f64((lane_base + (int)l_blocks[1 * nb + b]) << 2, cur_v) + lp_re);
            if (v > re) { re = v; re_bp = b; }
          }
          // run start {start state, run end}: the start state has a score in column 0 only (no predecessors, hmm_model.rs:91-94), so
          // from column 1 on its candidate is -inf + lp = -inf and loses the strict '>': the run start is what the run end gives
          double br = NINF; int pr = 0xFF;
          if constexpr (FIRST) {
            const double start_now = bperm_f64(a_st0, cur_v);
            const double v0 = (start_now + lp_rs0), v1 = (re + lp_rs1);
            if (v0 > br) { br = v0; pr = 0; }
            if (v1 > br) { br = v1; pr = 1; }
          } else {
            const double v1 = (re + lp_rs1);
            if (v1 > br) { br = v1; pr = 1; }
          }
          double msv = NINF; int ms_bp = 0xFF;  // the start of my block: {run start, own block end}
          {
            const double v0 = (br + ms_lp0), v1 = (myend + ms_lp1);
            if (v0 > msv) { msv = v0; ms_bp = 0; }
            if (v1 > msv) { msv = v1; ms_bp = 1; }
          }
          if (is_run_end) bpi = re_bp;
          if (is_run_start) bpi = pr;
          if (role_start) bpi = ms_bp;
          const double loc = loc_is_re ? re : msv;
          pe0 = use_loc0 ? loc : f0; pe1 = use_loc1 ? msv : f1; pe2 = f2; pe3 = f3;
        }
        HP_FILL(4);
        if (act) bp_col[st] = (uint8_t)bpi;  // (a uniform base that moves by a column, the lane's state as the offset: no 64-bit address arithmetic per lane)
        bp_col += Spad;
        HP_FILL(5);
      };
      column(0, std::true_type());
      for (int i = 1; i < L; ++i) column(i, std::false_type());
    } else {
    double prev_v = NINF;
    double em_next = 0.0;
    for (int i = 0; i < L; ++i) {
      if ((i % HMM_CODE_WINDOW) == 0) {
        hmm_sync(sync_n);
        win0 = i;
        for (int k = tid; k < HMM_CODE_WINDOW + 1 && i + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, i + k, L);
        hmm_sync(sync_n);
        sym_next = code_at(i);
        em_next = l_em[sym_next * S + st];
      }
      const double em = em_next;
      if (i + 1 < L) { sym_next = code_at(i + 1); em_next = l_em[sym_next * S + st]; }  // (a column ahead: off this column's critical path)
      HP_FILL(0);
      double best = NINF;
      int bpi = 0xFF;
      {
        const double s0 = bperm_f64(a_q0, prev_v), s1 = bperm_f64(a_q1, prev_v), s2 = bperm_f64(a_q2, prev_v), s3 = bperm_f64(a_q3, prev_v);
        if (act && level == 0) {
          if (i == 0) {
            if (n_in == 0 && em > NINF) { best = em; bpi = 0xFE; }  // the start state (hmm_model.rs:91-94)
          } else {
            const double v0 = (s0 + lp0) + em, v1 = (s1 + lp1) + em, v2 = (s2 + lp2) + em, v3 = (s3 + lp3) + em;
            if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
            if (n_in > 1 && v1 > best) { best = v1; bpi = 1; }
            if (n_in > 2 && v2 > best) { best = v2; bpi = 2; }
            if (n_in > 3 && v3 > best) { best = v3; bpi = 3; }
          }
        }
      }
      double cur_v = best;  // emitting states: final; silent ones: -inf until their pass
      HP_FILL(1);
      {  // the chains d0 <- d1 <- ... <- block end (see the LDS variant below for the argument)
        const double s0 = bperm_f64(a_q0, cur_v), s1 = bperm_f64(a_q1, cur_v);
        if (role_chain) {
          const double v0 = (s0 + lp0), v1 = (s1 + lp1);
          if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
          if (role_end && n_in > 1 && v1 > best) { best = v1; bpi = 1; }
        }
        double val = best, cand = NINF;
        for (int t = 0; wave_chain && t < chain_steps; ++t) {
          cand = (wave_shr1_f64(val) + lp_step);
          val = cand > best ? cand : best;
        }
        if (cand > best) bpi = role_del ? 1 : 2;  // (never for the lanes whose transition term is -inf)
        best = val;
        if (role_chain) cur_v = val;
      }
      HP_FILL(2);
      {  // run end: the block ends in block order; the run start {start state, run end} behind it -- by every lane, kept by the two
        const double start_now = bperm_f64(a_st0, cur_v);
        double re = NINF; int re_bp = 0xFF;
        auto block_ends = [&](auto n_const) {
          constexpr int N = decltype(n_const)::value;
          double e[N];
#pragma unroll
          for (int b = 0; b < N; ++b) e[b] = bperm_f64(a_be[b], cur_v);
#pragma unroll
          for (int b = 0; b < N; ++b) {
            const double v = (e[b] + lp_re);
            if (b < nb && v > re) { re = v; re_bp = b; }
          }
        };
        if (nb <= 2) block_ends(std::integral_constant<int, 2>());
        else if (nb <= 4) block_ends(std::integral_constant<int, 4>());
        else block_ends(std::integral_constant<int, BE_REG>());
        for (int b = BE_REG; b < nb; ++b) {
          const double v = (bperm_f64((lane_base + (int)l_blocks[1 * nb + b]) << 2, cur_v) + lp_re);
          if (v > re) { re = v; re_bp = b; }
        }
        double br = NINF; int pr = 0xFF;
        const double v0 = (start_now + lp_rs0), v1 = (re + lp_rs1);
        if (v0 > br) { br = v0; pr = 0; }
        if (v1 > br) { br = v1; pr = 1; }
        if (is_run_end) { cur_v = re; best = re; bpi = re_bp; }
        if (is_run_start) { cur_v = br; best = br; bpi = pr; }
      }
      HP_FILL(3);
      {  // block starts: {run start, own block end}
        const double s0 = bperm_f64(a_q0, cur_v), s1 = bperm_f64(a_q1, cur_v);
        if (role_start) {
          const double v0 = (s0 + lp0), v1 = (s1 + lp1);
          if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
          if (n_in > 1 && v1 > best) { best = v1; bpi = 1; }
          cur_v = best;
        }
      }
      HP_FILL(4);
      if (act) bp[(size_t)i * Spad + st] = (uint8_t)bpi;
      prev_v = cur_v;
      HP_FILL(5);
    }
    }
  } else if (two_rounds) {
    // The LDS fill with two barriers per column (plus one per extra chain round): emitting states | chains | -- and what used to be
    // two more passes with a barrier each (run end + run start by one lane, then the block starts) every lane works out for itself
    // from the block ends, the start state and its own block's end, as in the register fill above.  Run end, run start and block
    // starts are not written to the score columns any more: the only readers were those passes and the next column's emitting states,
    // which take them from their own copy.
    const double lp_re = l_lp[S - 2];
    const bool is_run_end = act && n_in == 0xFF, is_run_start = act && st == 1;
    const bool loc_is_re = act && use_loc0 && p0 == S - 2;
    double loc = NINF, msv_prev = NINF;  // my copies of the column before: run end or own block start | own block start
    uint8_t* __restrict__ bp_col = bp;
    for (int i = 0; i < L; ++i) {  // (column 0 as a copy of its own, as in the register fill, measured slower here: 5.45 -> 5.64 ms)
      if ((i % HMM_CODE_WINDOW) == 0) {
        hmm_sync(sync_n);
        win0 = i;
        for (int k = tid; k < HMM_CODE_WINDOW + 1 && i + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, i + k, L);
        hmm_sync(sync_n);
        sym_next = code_at(i);
      }
      const int sym = sym_next;
      if (i + 1 < L) sym_next = code_at(i + 1);
      HP_FILL(0);
      double best = NINF;
      int bpi = 0xFF;
      if (act && level == 0) {
        const double em = l_em[sym * S + st];
        if (i == 0) {
          if (n_in == 0 && em > NINF) { best = em; bpi = 0xFE; }  // the start state (hmm_model.rs:91-94)
        } else {
          const double r0 = prev[q0], r1 = prev[q1], s2 = prev[q2], s3 = prev[q3];
          const double s0 = use_loc0 ? loc : r0, s1 = use_loc1 ? msv_prev : r1;
          const double v0 = (s0 + lp0) + em, v1 = (s1 + lp1) + em, v2 = (s2 + lp2) + em, v3 = (s3 + lp3) + em;
          if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
          if (n_in > 1 && v1 > best) { best = v1; bpi = 1; }
          if (n_in > 2 && v2 > best) { best = v2; bpi = 2; }
          if (n_in > 3 && v3 > best) { best = v3; bpi = 3; }
        }
        cur[st] = best;
      }
      hmm_sync(sync_n);
      HP_FILL(1);
      if (role_chain) {
        const double s0 = cur[q0], s1 = cur[q1];
        const double v0 = (s0 + lp0), v1 = (s1 + lp1);
        if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
        if (role_end && n_in > 1 && v1 > best) { best = v1; bpi = 1; }
      }
      {
        const double own = best;
        int own_bp = bpi;
        double val = best, cand = NINF;
        for (int r = 0; r < chain_rounds; ++r) {
          if (chain_xwave) {
            cand = (cur[st - 1] + lp_chain);
            best = cand > own ? cand : own;
            bpi = cand > own ? (role_del ? 1 : 2) : own_bp;
            val = best;
          }
          for (int t = 0; wave_chain && t < chain_steps; ++t) {
            cand = (wave_shr1_f64(val) + lp_step);
            val = max_f64(cand, best);
          }
          if (role_chain) cur[st] = val;
          if (r + 1 < chain_rounds) hmm_sync(sync_n);
        }
        if (cand > best) bpi = role_del ? 1 : 2;
        best = val;
      }
      hmm_sync(sync_n);
      HP_FILL(2);
      {
        const double myend = cur[my_me];
        double re = NINF; int re_bp = 0xFF;
        auto block_ends = [&](auto n_const) {
          constexpr int N = decltype(n_const)::value;
          double e[N];
#pragma unroll
          for (int b = 0; b < N; ++b) e[b] = cur[be[b]];
#pragma unroll
          for (int b = 0; b < N; ++b) {
            const double v = (e[b] + lp_re);
            if (b < nb && v > re) { re = v; re_bp = b; }
          }
        };
        if (nb <= 2) block_ends(std::integral_constant<int, 2>());
        else if (nb <= 4) block_ends(std::integral_constant<int, 4>());
        else block_ends(std::integral_constant<int, BE_REG>());
        for (int b = BE_REG; b < nb; ++b) {
          const double v = (cur[l_blocks[1 * nb + b]] + lp_re);
          if (v > re) { re = v; re_bp = b; }
        }
        double br = NINF; int pr = 0xFF;  // (the start state has a score in column 0 only: see the register fill)
        if (i == 0) {
          const double start_now = cur[0];
          const double v0 = (start_now + lp_rs0), v1 = (re + lp_rs1);
          if (v0 > br) { br = v0; pr = 0; }
          if (v1 > br) { br = v1; pr = 1; }
        } else {
          const double v1 = (re + lp_rs1);
          if (v1 > br) { br = v1; pr = 1; }
        }
        double msv = NINF; int ms_bp = 0xFF;  // the start of my block: {run start, own block end}
        {
          const double v0 = (br + ms_lp0), v1 = (myend + ms_lp1);
          if (v0 > msv) { msv = v0; ms_bp = 0; }
          if (v1 > msv) { msv = v1; ms_bp = 1; }
        }
        if (is_run_end) bpi = re_bp;
        if (is_run_start) bpi = pr;
        if (role_start) bpi = ms_bp;
        loc = loc_is_re ? re : msv; msv_prev = msv;
      }
      HP_FILL(4);
      if (act) bp_col[st] = (uint8_t)bpi;
      bp_col += Spad;
      double* t = prev; prev = cur; cur = t;
      HP_FILL(5);
    }
  } else
  for (int i = 0; i < L; ++i) {
    if ((i % HMM_CODE_WINDOW) == 0) {  // next window of symbol codes (one column more than the window: the look-ahead below)
      hmm_sync(sync_n);
      win0 = i;
      for (int k = tid; k < HMM_CODE_WINDOW + 1 && i + k < L; k += nthr) l_seq[k] = (uint8_t)hmm_code(seq, i + k, L);
      hmm_sync(sync_n);
      sym_next = code_at(i);
    }
    const int sym = sym_next;
    if (i + 1 < L) sym_next = code_at(i + 1);  // (fetched a column ahead: its LDS round trip is off this column's critical path)
    HP_FILL(0);
    double best = NINF;
    int bpi = 0xFF;
    if (act && level == 0) {
      const double em = l_em[sym * S + st];
      if (i == 0) {
        if (n_in == 0 && em > NINF) { best = em; bpi = 0xFE; }  // the start state (hmm_model.rs:91-94)
      } else {
        // all four predecessor scores are fetched first (one LDS wait instead of four); same sums, same strict '>' in the same order
        const double s0 = prev[q0], s1 = prev[q1], s2 = prev[q2], s3 = prev[q3];
        const double v0 = (s0 + lp0) + em, v1 = (s1 + lp1) + em, v2 = (s2 + lp2) + em, v3 = (s3 + lp3) + em;
        if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
        if (n_in > 1 && v1 > best) { best = v1; bpi = 1; }
        if (n_in > 2 && v2 > best) { best = v2; bpi = 2; }
        if (n_in > 3 && v3 > best) { best = v3; bpi = 3; }
      }
      cur[st] = best;
    }
    hmm_sync(sync_n);
    HP_FILL(1);
    // (Silent states emit nothing: the reference adds an emission term of 0.0 to their sums, which changes no value -- scores are sums of
    //  logarithms of probabilities, never -0.0 -- and is left out here.)
    // Silent states of the column in three passes instead of one per topological level (motif length + 3 of them).  First the chains
    // d0 <- d1 <- ... <- block end of all motif blocks at once: a chain state is max(what its other predecessors give, the state before
    // it + lp) with ties to the former, and the state before it is the LANE before it -- every lane takes its neighbour's value
    // (DPP wave_shr:1: no LDS round trip), and after k steps the k-th state of a chain has its final value (steps beyond that
    // recompute it from the same inputs).  A chain that runs over a wave boundary takes another round: the first lane of a wave reads
    // the state before it from LDS.  Then the run-end lane takes the maximum over the block ends and evaluates the run start behind
    // it; then every block start.  Same sums, same predecessor order, same strict '>' as level by level (any topological order gives
    // identical values, hmm_model.rs:206-240).
    if (role_chain) {
      const double s0 = cur[q0], s1 = cur[q1];
      const double v0 = (s0 + lp0), v1 = (s1 + lp1);
      if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
      if (role_end && n_in > 1 && v1 > best) { best = v1; bpi = 1; }
    }
    {
      const double own = best;  // what the predecessors other than the chain's give
      int own_bp = bpi;
      double val = best, cand = NINF;
      for (int r = 0; r < chain_rounds; ++r) {
        if (chain_xwave) {  // the state before sits in the wave before: final after the round before (round 0: a throw-away value)
          cand = (cur[st - 1] + lp_chain);
          best = cand > own ? cand : own;
          bpi = cand > own ? (role_del ? 1 : 2) : own_bp;
          val = best;
        }
        for (int t = 0; wave_chain && t < chain_steps; ++t) {
          cand = (wave_shr1_f64(val) + lp_step);
          val = cand > best ? cand : best;
        }
        if (role_chain) cur[st] = val;
        if (r + 1 < chain_rounds) hmm_sync(sync_n);
      }
      if (cand > best) bpi = role_del ? 1 : 2;  // (never for the lanes whose transition term is -inf)
      best = val;
    }
    hmm_sync(sync_n);
    HP_FILL(2);
    if (act && n_in == 0xFF) {  // run end: block ends in block order; then the run start {start state, run end}
      const double start_now = cur[0];  // (the start state of this column, for the run start below: fetched with the block ends)
      // (their indices sit in registers: one round trip for all of them; a model of one or two motifs -- two or three blocks, nearly every
      //  locus of a genome-wide catalog -- fetches and compares only what it has: 8 fetches and compares per column were 200 of its 2 400 cycles)
      auto block_ends = [&](auto n_const) {
        constexpr int N = decltype(n_const)::value;
        double e[N];
#pragma unroll
        for (int b = 0; b < N; ++b) e[b] = cur[be[b]];
#pragma unroll
        for (int b = 0; b < N; ++b) {
          const double v = (e[b] + lp0);
          if (b < nb && v > best) { best = v; bpi = b; }
        }
      };
      if (nb <= 2) block_ends(std::integral_constant<int, 2>());
      else if (nb <= 4) block_ends(std::integral_constant<int, 4>());
      else block_ends(std::integral_constant<int, BE_REG>());
      for (int b = BE_REG; b < nb; ++b) {
        const double v = (cur[l_blocks[1 * nb + b]] + lp0);
        if (v > best) { best = v; bpi = b; }
      }
      cur[st] = best;
      double br = NINF; int pr = 0xFF;
      const double v0 = (start_now + lp_rs0), v1 = (best + lp_rs1);
      if (v0 > br) { br = v0; pr = 0; }
      if (v1 > br) { br = v1; pr = 1; }
      cur[1] = br; l_bpcol[1] = (uint8_t)pr;
    }
    hmm_sync(sync_n);
    HP_FILL(3);
    if (role_start) {  // block start: {run start, own block end}
      const double s0 = cur[q0], s1 = cur[q1];
      const double v0 = (s0 + lp0), v1 = (s1 + lp1);
      if (n_in > 0 && v0 > best) { best = v0; bpi = 0; }
      if (n_in > 1 && v1 > best) { best = v1; bpi = 1; }
      cur[st] = best;
    }
    hmm_sync(sync_n);
    HP_FILL(4);
    if (act && st == 1) bpi = l_bpcol[1];  // the run start was evaluated by the run-end lane
    if (act) bp[(size_t)i * Spad + st] = (uint8_t)bpi;
    double* t = prev; prev = cur; cur = t;
    HP_FILL(5);
  }
  }  // (fill)
  HP_FILL_END;
  HP_MARK(1);
  // long alleles are traced back by hmm_traceback_long_kernel (many waves per allele, behind this launch on the same stream)
  if (long_list && job.map_off && L >= long_min) {
    hmm_sync_mem(sync_n);
    if (tid == 0) long_list[1 + atomicAdd(long_list, 1u)] = jidx;
    return;
  }
  if (tid == 0) hmm_trace_init(tb, S, L);
  hmm_sync_mem(sync_n);  // the back-pointer columns written by all waves are read back from here on

  // ---- traceback, fused with the events, the purity counts and the motif-visit collection (hmm_traceback.hpp).
  // rows of the back-pointer workspace: one byte per state (this kernel's own fill, the round-5 layout of the position-per-lane fill) or
  // one byte per lane of the job's group (hmm_fill_ppl_kernel<G, true>)
  const bool packed = ppl_filled && ppl_packed && set.ppl_lanes != 0u;
  const int rstride = packed ? hmm_ppl_group(set.ppl_lanes) : Spad;
  const int cols_per_chunk = packed ? hmm_stage_bytes(Spad) / rstride - 2 : max(1, hmm_stage_bytes(Spad) / Spad);
  if (tid == 0) tb[TB_LOC] = 0;  // (the end state: a constant 0)
  uint16_t* pbuf = path ? path + job.path_off : nullptr;
  uint32_t* const g_vis = visit_ws + job.visit_off;  // visits HMM_VIS_LDS, HMM_VIS_LDS + 1, ... at their own index
  const int pcap = (int)job.path_cap;
  constexpr int HMM_REC = SUB == 32 ? 32 : 64;  // steps per round: the lanes of the job's first wave
  const unsigned long long gmask = SUB == 32 ? (0xFFFFFFFFull << (threadIdx.x & 32u)) : ~0ull;  // the lanes of my job in this wave
  const HmmSyncN sync{sync_n};
  const HmmTraceLds tl{tb, l_inst, l_info, l_blocks, l_flags, l_stage, l_seq, l_mot, l_vis, l_cnt, l_rec};
  hmm_trace_rounds<HMM_REC, true>(sync, tid, nthr, tl, packed, rstride, cols_per_chunk, S, nb, L, seq, bp, g_vis, pbuf, pcap, gmask);
  const int np = tb[TB_NPATH];
  HP_MARK(2);
  hmm_path_to_front(sync, tid, nthr, pbuf, np, pcap);
  if (tid == 0) hmm_store_purity(job.job_index, np, tb[TB_EDIT], tb[TB_REF], qlen, path_len, purity, edit_out, maxd_out);
  hmm_decode_visits(sync, tid, nthr, tl, nb, g_vis, spans3 + 3 * job.span_off, n_spans + job.job_index, counts + job.count_off);
  HP_MARK(3);
}

#include "hmm_ppl.hpp"
#include "hmm_trace_ppl.hpp"
#include "hmm_big.hpp"

// ---- trace-back of LONG alleles on many waves (DESIGN_HISTORY 7.3: "block-wise composed trace-back").  The chase of the back-pointers
// is a serial chain of dependent look-ups -- a third of a long allele's time on one lane.  Here the columns are cut into chunks of
// HMM_LONG_CHUNK; (A) for every chunk and EVERY state it could be entered in, a wave (lane = entry state) walks the chunk and notes where
// the walk leaves it and what it passed (steps, motif visits, the last block end, the last state); (B) one thread strings the chunks
// together from the end state -- a look-up per chunk; (C) every chunk is walked again from its now known entry state with the full
// decoding of the steps (events, purity counts, motif visits: the code of hmm_viterbi_kernel), the waves of the workgroup side by side.
// Exact by construction: (C) walks the very path the serial chase walks, and what a step needs from the steps before it (the state
// walked last, the column of the last block end, how many steps / visits came before) is handed over by (B).
struct HmmChunkMap { uint16_t exit_state, last_state, n_steps, n_starts; int32_t last_end; };  // 12 bytes = 3 words
struct HmmChunkRec { uint32_t entry, np0, nv0; int32_t vb0, nxt0; uint32_t pad[3]; };          // 8 words
constexpr int HMM_LONG_THREADS = 1024, HMM_LONG_STG = 2048;
constexpr int HMM_LONG_MAP_LDS = 48 * 1024;  // chunk maps and records that fit stay in LDS (a 10-kb allele of a 16-state model: 35 KB), else in the job's workspace

__global__ void __launch_bounds__(HMM_LONG_THREADS) hmm_traceback_long_kernel(
    const HmmJobDev* __restrict__ jobs, const HmmSetDev* __restrict__ sets, const uint8_t* __restrict__ model, const uint8_t* __restrict__ seq_blob,
    const uint8_t* __restrict__ bp_ws, uint32_t* __restrict__ visit_ws, uint16_t* __restrict__ path, uint32_t* __restrict__ path_len,
    int32_t* __restrict__ spans3, uint32_t* __restrict__ n_spans, uint32_t* __restrict__ counts, double* __restrict__ purity,
    int32_t* __restrict__ edit_out, int32_t* __restrict__ maxd_out, const uint32_t* __restrict__ long_list, const int phase_arg, const int G) {
  const int phase = phase_arg & 0xFF;
  const bool ppl_packed = ((phase_arg >> 8) & 1) != 0;  // the position-per-lane fill wrote rows of one byte per lane (hmm_fill_ppl_kernel<G, true>)
  // phase 0: the whole trace-back by one workgroup per allele.  Phases 1 / 2 / 3 are the same code as three launches with G workgroups
  // per allele in (A) and (C) -- an allele's chunks are independent there, and a class has few long alleles for 256 CUs: 1: (A) with
  // the maps in the job's workspace; 2: (B) by one workgroup; 3: (C), the totals in the four words in front of the maps, and the
  // workgroup that finishes last does the rest (path order, purity, visits).
  extern __shared__ __align__(16) unsigned char lds_long[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = HMM_LONG_THREADS / 64;
  const int part = (int)(blockIdx.x % (unsigned)G);
  __shared__ int l_last;
  for (uint32_t li = blockIdx.x / (unsigned)G; li < long_list[0]; li += gridDim.x / (unsigned)G) {
    __syncthreads();
    const HmmJobDev job = jobs[long_list[1 + li]];
    const HmmSetDev set = sets[job.set];
    const int S = (int)set.S, nb = (int)set.n_blocks, n_motifs = nb - 1;
    const int qlen = (int)job.seq_len, L = qlen + 2;
    const int Spad = (S + 15) & ~15;
    const int C = HMM_LONG_CHUNK, n_chunks = (L + C - 1) / C;
    // ---- LDS: totals | tables | per wave: staged back-pointer columns, the steps of a round
    int* tot = reinterpret_cast<int*>(lds_long);  // [0] edit, [1] ref, [2] np, [3] nv
    uint32_t* l_inst = reinterpret_cast<uint32_t*>(lds_long + 64);                       // [S][4] hmm_pred_entry
    uint32_t* l_info = l_inst + 4 * S;                                                   // [S]
    uint32_t* l_blocks = l_info + S;                                                     // [4][nb]
    uint32_t* l_cnt = l_blocks + 4 * nb;                                                 // [nb]
    uint8_t* l_flags = reinterpret_cast<uint8_t*>(l_cnt + nb);                           // [S]
    const int mot_bytes = (S - 7 - n_motifs) / 3;
    uint8_t* l_mot = l_flags + ((S + 3) & ~3);
    unsigned char* wave_base = lds_long + ((64 + (size_t)16 * S + 4 * S + 16 * nb + 4 * nb + ((S + 3) & ~3) + ((mot_bytes + 15) & ~15) + 15) & ~(size_t)15);
    uint8_t* l_stage = wave_base + (size_t)wave * (HMM_LONG_STG + 512);
    uint32_t* const l_map = reinterpret_cast<uint32_t*>(wave_base + (size_t)NW * (HMM_LONG_STG + 512));
    const bool map_lds = phase == 0 && ((size_t)3 * S + 8) * (size_t)n_chunks * 4 <= (size_t)HMM_LONG_MAP_LDS;
    uint32_t* const hdr = visit_ws + job.map_off - 4;                                    // [0] edit, [1] ref, [2] workgroups done (phase 3)
    uint32_t* l_rec = reinterpret_cast<uint32_t*>(l_stage + HMM_LONG_STG);               // [64][2]
    const uint16_t* g_inst = reinterpret_cast<const uint16_t*>(model + set.off_inst);
    const int16_t* g_block = reinterpret_cast<const int16_t*>(model + set.off_block);
    const uint32_t* g_blocks = reinterpret_cast<const uint32_t*>(model + set.off_blocks);
    const uint8_t* g_motifs = model + set.off_motifs;
    for (int i = tid; i < 4 * S; i += HMM_LONG_THREADS) l_inst[4 * (i % S) + i / S] = hmm_pred_entry(g_inst[i], S, nb, model + set.off_flags, g_block, g_blocks);
    for (int i = tid; i < S; i += HMM_LONG_THREADS) l_flags[i] = model[set.off_flags + i];
    for (int i = tid; i < 4 * nb; i += HMM_LONG_THREADS) l_blocks[i] = g_blocks[i];
    for (int i = tid; i < mot_bytes; i += HMM_LONG_THREADS) l_mot[i] = g_motifs[i];
    for (int i = tid; i < nb; i += HMM_LONG_THREADS) l_cnt[i] = 0;
    for (int m = tid; m < n_motifs; m += HMM_LONG_THREADS) counts[job.count_off + m] = 0;
    if (tid < 4) tot[tid] = 0;
    __syncthreads();
    for (int st = tid; st < S; st += HMM_LONG_THREADS) {  // the trace-back word of a state (as in hmm_viterbi_kernel)
      const int blk = (int)g_block[st];
      uint32_t kind = 0, expected = 0;
      if (blk >= 0) {
        const int bstart = (int)l_blocks[0 * nb + blk], bend = (int)l_blocks[1 * nb + blk];
        if (st == bstart) kind = 1;
        else if (st == bend) kind = 2;
        else if (blk == nb - 1) kind = 3;
        else {
          const int mlen = (int)l_blocks[2 * nb + blk], off = st - bstart - 1, k = off / mlen;
          kind = 4u + (uint32_t)k;
          if (k == 0) expected = l_mot[l_blocks[3 * nb + blk] + off];
        }
      }
      l_info[st] = kind | ((uint32_t)(l_flags[st] & 1) << 3) | ((uint32_t)(blk & 0xFF) << 8) | (expected << 16);
    }
    __syncthreads();
    const uint8_t* __restrict__ seq = seq_blob + job.seq_off;
    const uint8_t* __restrict__ bp = bp_ws + job.bp_off;
    uint32_t* const g_vis = visit_ws + job.visit_off;
    uint32_t* const g_map = map_lds ? l_map : visit_ws + job.map_off;                 // [n_chunks][S] HmmChunkMap
    HmmChunkRec* const g_crec = reinterpret_cast<HmmChunkRec*>(g_map + (size_t)3 * S * n_chunks);  // [n_chunks]
    const bool packed = ppl_packed && set.ppl_lanes != 0u;
    const int rstride = packed ? hmm_ppl_group(set.ppl_lanes) : Spad;   // bytes per column (rows of one byte per state, or per lane of the job's group)
    const int sub_cols = max(1, HMM_LONG_STG / rstride);
    // the back-pointer of `state` (loc: its hmm_bp_loc) in the staged row at `row`
    auto bp_at = [&](int row, int state, uint32_t loc) -> int {
      if (!packed) return (int)l_stage[row + state];
      if (state == S - 2) return (int)hmm_bp_run_end(*reinterpret_cast<const uint32_t*>(l_stage + row));
      return (int)hmm_bp_unpack(l_stage[row + (int)(loc & 63u)], loc);
    };
    // one step of the chase: the predecessor of `state` in column `idx` (b: its back-pointer)
    // (all four predecessor entries of the state are read before its back-pointer is known -- one LDS round trip per step, not two)
    auto pred_of = [&](int state, int b, const uint4& p4) -> uint32_t {
      uint32_t pe = (b & 2) ? ((b & 1) ? p4.w : p4.z) : ((b & 1) ? p4.y : p4.x);
      if (state == S - 2) { const int bb = b < nb ? b : 0; const uint32_t be_ = l_blocks[1 * nb + bb]; pe = be_ | ((uint32_t)(l_flags[be_] & 1) << 15) | (hmm_bp_loc_block_end(bb, nb, l_blocks) << 16); }
      return pe;
    };
    // wave-cooperative staging of the back-pointer columns [c0, c1) (16-byte pieces; c0 is a multiple of the chunk length: 16-byte aligned rows)
    auto stage_cols = [&](int c0, int c1) {
      const uint4* src = reinterpret_cast<const uint4*>(bp + (size_t)c0 * rstride);
      uint4* dst = reinterpret_cast<uint4*>(l_stage);
      const int n16 = ((c1 - c0) * rstride + 15) / 16;
      for (int i = lane; i < n16; i += 64) dst[i] = src[i];
    };
    HP_LONG_DECL;
    // ---- (A) chunk maps: every (chunk, block of 64 entry states) is a task of one wave
    const int passes = (S + 63) / 64;
    if (phase <= 1)
    for (int task = wave + NW * part; task < n_chunks * passes; task += NW * G) {
      const int j = task / passes, q = task % passes;
      const int bot = j * C, top = min(L - 1, bot + C - 1);
      const int s0 = 64 * q + lane;
      int state = s0 < S ? s0 : 0, idx = top;
      uint32_t loc = packed && s0 < S ? hmm_bp_loc(s0, nb, (int)g_block[s0], l_blocks) : 0u;
      int nsteps = 0, nstarts = 0, last_end = -1, last_state = state;
      const int step_cap = (top - bot + 1) * (int)(set.max_mlen + 8) + S;  // (entry states the path cannot be in may hold arbitrary back-pointers)
      for (int c1 = top + 1; c1 > bot;) {
        const int c0 = max(bot, c1 - sub_cols);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        stage_cols(c0, c1);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        while (__ballot(state != 0 && idx >= c0 && nsteps < step_cap) != 0ull) {
          if (state != 0 && idx >= c0 && nsteps < step_cap) {
            const uint4 p4 = *reinterpret_cast<const uint4*>(l_inst + 4 * state);
            const uint32_t inf = l_info[state];
            const int b = bp_at((idx - c0) * rstride, state, loc);
            const int kind = (int)(inf & 7u);
            ++nsteps; nstarts += kind == 1; if (kind == 2) last_end = idx; last_state = state;
            const uint32_t pe = pred_of(state, b, p4);
            if ((inf >> 3) & 1u) --idx;
            const int nx = (int)(pe & 0x7FFFu);
            state = nx < S ? nx : 0;
            loc = nx < S ? pe >> 16 : 0u;
          }
        }
        c1 = c0;
      }
      if (s0 < S) {
        uint32_t* m = g_map + (size_t)3 * ((size_t)j * S + s0);
        m[0] = (uint32_t)(nsteps >= step_cap ? 0 : state) | ((uint32_t)last_state << 16);
        m[1] = (uint32_t)(nsteps & 0xFFFF) | ((uint32_t)(nstarts & 0xFFFF) << 16);
        m[2] = (uint32_t)last_end;
      }
    }
    __syncthreads();  // (+ the maps are in global memory: read back by thread 0 of this workgroup)
    __threadfence();
    HP_LONG(4);
    if (phase == 1) continue;
    // ---- (B) the chunks strung together from the end state
    uint32_t* const g_tail = reinterpret_cast<uint32_t*>(g_crec + n_chunks);  // [0] steps, [1] visits of the whole walk (phases 2 -> 3)
    if (phase == 2 && (size_t)3 * S * (size_t)n_chunks * 4 <= (size_t)HMM_LONG_MAP_LDS) {  // the maps through LDS: the chain is a dependent look-up per chunk
      for (int i = tid; i < 3 * S * n_chunks; i += HMM_LONG_THREADS) l_map[i] = __builtin_nontemporal_load(g_map + i);
      __syncthreads();
    }
    const bool b_lds = map_lds || (phase == 2 && (size_t)3 * S * (size_t)n_chunks * 4 <= (size_t)HMM_LONG_MAP_LDS);
    if (tid == 0 && phase != 3) {
      uint32_t e = (uint32_t)(S - 1), np = 0, nv = 0; int vb = 0, nxt = -1;
      for (int j = n_chunks - 1; j >= 0; --j) {
        HmmChunkRec r; r.entry = e; r.np0 = np; r.nv0 = nv; r.vb0 = vb; r.nxt0 = nxt; r.pad[0] = r.pad[1] = r.pad[2] = 0;
        g_crec[j] = r;
        const uint32_t* m = (b_lds ? l_map : g_map) + (size_t)3 * ((size_t)j * S + e);
        const uint32_t m0 = b_lds ? m[0] : __builtin_nontemporal_load(m), m1 = b_lds ? m[1] : __builtin_nontemporal_load(m + 1), m2 = b_lds ? m[2] : __builtin_nontemporal_load(m + 2);
        const uint32_t ns = m1 & 0xFFFFu;
        np += ns; nv += m1 >> 16;
        if ((int32_t)m2 >= 0) vb = (int32_t)m2;
        if (ns) nxt = (int)(m0 >> 16);
        e = m0 & 0xFFFFu;
      }
      tot[2] = (int)np; tot[3] = (int)nv;
      if (phase == 2) { g_tail[0] = np; g_tail[1] = nv; hdr[0] = 0; hdr[1] = 0; hdr[2] = 0; }
    }
    __syncthreads();
    __threadfence();
    HP_LONG(5);
    if (phase == 2) continue;
    // ---- (C) every chunk again, from its entry state, with the decoding of the steps (the round loop of hmm_viterbi_kernel)
    uint16_t* pbuf = path ? path + job.path_off : nullptr;
    const int pcap = (int)job.path_cap;
    auto code_at = [&](int i) -> int { return hmm_code(seq, i, L); };
    int edit_acc = 0, ref_acc = 0;
    for (int j = wave + NW * part; j < n_chunks; j += NW * G) {
      const HmmChunkRec cr = g_crec[j];
      const int bot = j * C, top = min(L - 1, bot + C - 1);
      int state = (int)cr.entry, idx = top, np_c = (int)cr.np0, nv_c = (int)cr.nv0, vb_c = cr.vb0, nxt_c = cr.nxt0;
      uint32_t loc = packed && state < S ? hmm_bp_loc(state, nb, (int)g_block[state], l_blocks) : 0u;
      for (int c1 = top + 1; c1 > bot && state != 0;) {
        const int c0 = max(bot, c1 - sub_cols);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        stage_cols(c0, c1);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        while (state != 0 && idx >= c0) {
          // the chase of up to 64 steps: on wave-uniform values (state and column in SGPRs: scalar arithmetic, scalar branches)
          int n = 0;
          int emits = __builtin_amdgcn_readfirstlane((int)((l_info[state] >> 3) & 1u));  // (afterwards: bit 15 of the predecessor entry)
          while (state != 0 && idx >= c0 && n < 64) {
            l_rec[2 * n] = (uint32_t)state; l_rec[2 * n + 1] = (uint32_t)idx; ++n;
            const uint4 p4 = *reinterpret_cast<const uint4*>(l_inst + 4 * state);
            const int b = __builtin_amdgcn_readfirstlane(bp_at((idx - c0) * rstride, state, loc));
            const uint32_t pe = (uint32_t)__builtin_amdgcn_readfirstlane((int)pred_of(state, b, p4));
            if (emits) --idx;
            emits = (int)((pe >> 15) & 1u);
            state = (int)(pe & 0x7FFFu);
            loc = pe >> 16;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          {  // ---- what the noted steps mean, one lane per step; the visits always go to the job's workspace
            const HmmStepSums r = hmm_decode_steps<64>(lane, n, HmmStepCarry{np_c, nv_c, nxt_c, vb_c}, ~0ull, l_rec, l_info, l_blocks, nb, l_mot, pbuf, pcap, code_at,
                                                       [&](int nv) -> uint32_t* { return g_vis + 3 * (size_t)nv; });
            np_c += n; nv_c += r.n_starts; edit_acc += r.edit; ref_acc += r.ref;
            if (n > 0) nxt_c = r.last_state;
            if (r.any_end) vb_c = r.idx_last_end;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        c1 = c0;
      }
    }
    if (lane == 0) { atomicAdd(&tot[0], edit_acc); atomicAdd(&tot[1], ref_acc); }
    __syncthreads();
    __threadfence();
    HP_LONG(6);
    if (phase == 3) {  // totals of all workgroups of the allele; the one that arrives last goes on
      if (tid == 0) {
        atomicAdd(hdr + 0, (uint32_t)tot[0]); atomicAdd(hdr + 1, (uint32_t)tot[1]);
        __threadfence();
        l_last = atomicAdd(hdr + 2, 1u) == (uint32_t)(G - 1) ? 1 : 0;
      }
      __syncthreads();
      if (!l_last) continue;
      __threadfence();
      if (tid == 0) {
        tot[0] = (int)__hip_atomic_load(hdr + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); tot[1] = (int)__hip_atomic_load(hdr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tot[2] = (int)__builtin_nontemporal_load(g_tail); tot[3] = (int)__builtin_nontemporal_load(g_tail + 1);
      }
      __syncthreads();
    }
    // ---- the end of the walk (the start state closes the path), then as in hmm_viterbi_kernel: path order, purity, the visits
    int np = tot[2];
    if (tid == 0 && pbuf && np < pcap) pbuf[pcap - 1 - np] = 0;
    ++np;
    hmm_path_to_front(HmmSyncBlock{}, tid, HMM_LONG_THREADS, pbuf, np, pcap);
    if (tid == 0) hmm_store_purity(job.job_index, np, tot[0], tot[1], qlen, path_len, purity, edit_out, maxd_out);
    // label_motifs over the kept copies, skip filter, counts, collapse (hmm_model.rs:158-200, operations.rs:6-80, utils.rs:3-27), all threads:
    // the visits were recorded back to front, one lane takes one visit; base ranges by a prefix sum of the copy lengths, "the kept
    // visit before me" by a look-back (a span goes on when that one has my motif and ends where I start), span numbers by a prefix
    // count of the span heads, span ends by an atomic max (they grow along a span).  (One thread walking the list paid three
    // dependent global loads per visit: 43 % of this kernel on a 10-kb CAG allele.)
    {
      int32_t* const sp = spans3 + 3 * job.span_off;
      int* const sc_sum = reinterpret_cast<int*>(wave_base);  // [NW] | [NW] | [NW][3]: the staging areas are free now
      int* const sc_heads = sc_sum + NW;
      int* const sc_last = sc_heads + NW;
      const int nvis = tot[3];
      int carry_cum = 0, carry_ns = 0, carry_motif = -1, carry_end = -1;  // (the same in every thread)
      const unsigned long long below_m = (1ull << lane) - 1ull;
      auto scan_add = [&](int x, int* lds_w, int& total) -> int {  // inclusive prefix sum over the workgroup
        int v = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o); if (lane >= o) v += t; }
        if (lane == 63) lds_w[wave] = v;
        __syncthreads();
        int woff = 0, tt = 0;
        for (int w = 0; w < NW; ++w) { const int t = lds_w[w]; if (w < wave) woff += t; tt += t; }
        __syncthreads();
        total = tt;
        return v + woff;
      };
      for (int base = 0; base < nvis; base += HMM_LONG_THREADS) {
        const int i = base + tid;
        const bool in = i < nvis;
        uint32_t v0 = 0, v1 = 0, v2 = 0;
        if (in) {
          const uint32_t* vr = g_vis + 3 * (size_t)(nvis - 1 - i);
          v0 = __builtin_nontemporal_load(vr); v1 = __builtin_nontemporal_load(vr + 1); v2 = __builtin_nontemporal_load(vr + 2);
        }
        const int blk = (int)(v0 & 0x7FFFu), cnt = in ? (int)v2 - (int)v1 : 0;
        const int motif = (v0 >> 15) == 0 ? blk : nb - 1;
        const bool valid = in && motif < n_motifs;
        int total_cnt = 0;
        const int end = carry_cum + scan_add(cnt, sc_sum, total_cnt), start = end - cnt;
        // the kept visit before me: in my wave, else the last one of the nearest wave before that has any, else the chunk before
        const unsigned long long vm = __ballot(valid);
        const int last_lane = vm ? 63 - (int)__builtin_clzll(vm) : 0;
        if (lane == last_lane) { sc_last[3 * wave] = vm ? 1 : 0; sc_last[3 * wave + 1] = motif; sc_last[3 * wave + 2] = end; }
        __syncthreads();
        const unsigned long long vb = vm & below_m;
        const int src = vb ? 63 - (int)__builtin_clzll(vb) : lane;
        int pm = __shfl(motif, src), pe = __shfl(end, src);
        if (!vb) {
          pm = carry_motif; pe = carry_end;
          for (int w = wave - 1; w >= 0; --w) if (sc_last[3 * w]) { pm = sc_last[3 * w + 1]; pe = sc_last[3 * w + 2]; break; }
        }
        int new_motif = carry_motif, new_end = carry_end;
        for (int w = NW - 1; w >= 0; --w) if (sc_last[3 * w]) { new_motif = sc_last[3 * w + 1]; new_end = sc_last[3 * w + 2]; break; }
        const bool head = valid && !(pm == motif && pe == start && pm >= 0);
        int total_heads = 0;
        const int hincl = scan_add(head ? 1 : 0, sc_heads, total_heads);
        const int si = carry_ns + hincl - 1;  // my span (a head: the one it opens)
        if (head) { sp[3 * si + 0] = motif; sp[3 * si + 1] = start; sp[3 * si + 2] = end; }
        if (valid) atomicAdd(&l_cnt[motif], 1u);
        __syncthreads();
        __threadfence();
        if (valid && !head) atomicMax(&sp[3 * si + 2], end);
        carry_cum += total_cnt; carry_ns += total_heads; carry_motif = new_motif; carry_end = new_end;
        __syncthreads();
      }
      if (tid == 0) n_spans[job.job_index] = (uint32_t)carry_ns;
    }
    __syncthreads();
    for (int m = tid; m < n_motifs; m += HMM_LONG_THREADS) counts[job.count_off + m] = l_cnt[m];
    HP_LONG(7);
  }
}

// Job list of a launch class resolved on the device: candidate (locus, allele) slots with everything the host knows ahead of the
// genotyper (motif set, where the allele will be, output places, workspace for its longest possible sequence) become jobs once the
// genotyper has written how many alleles a locus has and how long they are -- no host round trip between the genotyper and this
// kernel's launch.  One workgroup per launch class (results land at the slot's index: the host needs no job order).
struct HmmResolveArgs {
  const HmmJobDev* cand; uint32_t n;
  const uint8_t* skip_locus; const int32_t* n_alleles; const uint32_t* allele_len;  // genotyper results (device), by locus / slot
  HmmJobDev* jobs; uint32_t* n_jobs; uint32_t* n_spans; double* purity;
  uint32_t len_shift;  // alleles are binned by length >> len_shift (64 bins, the last one open)
};
// ... longest alleles first (bins of similar length, descending): workgroups start in list order and a launch ends with its last
// allele -- a long allele started behind thousands of short ones is pure tail.  Three sweeps over the candidates: count per bin,
// exclusive scan over the bins from the longest down, scatter (the order inside a bin is whatever the atomics make it; results do
// not depend on the job order).
constexpr uint32_t HMM_RESOLVE_LDS = 24576;  // candidates whose (active, length) verdict is kept in LDS between the sweeps (96 KB)
__global__ void __launch_bounds__(1024) hmm_resolve_kernel(const HmmResolveArgs a) {
  __shared__ uint32_t hist[64], cursor[64];
  __shared__ uint32_t verdict[HMM_RESOLVE_LDS];  // length + 1 of an active candidate, 0 otherwise
  const int tid = (int)threadIdx.x;
  if (tid < 64) hist[tid] = 0;
  __syncthreads();
  auto probe = [&](uint32_t i) -> uint32_t {  // length + 1 if candidate i is a job, else 0
    const uint32_t slot = a.cand[i].job_index, l = slot >> 1, al = slot & 1u;
    const bool on = !a.skip_locus[l] && (int32_t)al < a.n_alleles[l];
    if (!on) { a.n_spans[slot] = 0; a.purity[slot] = __builtin_nan(""); }  // what the caller's arrays hold for an allele that is not there
    return on ? a.allele_len[slot] + 1u : 0u;
  };
  auto bin_of = [&](uint32_t len) { const uint32_t b = len >> a.len_shift; return 63u - (b < 63u ? b : 63u); };  // bin 0 = the longest
  // One LDS atomic per wave and bin, not per candidate: the alleles of an STR catalog fall into two or three bins, and 20 k atomics on
  // three LDS words were most of this kernel's 0.14 ms (it sits between the genotyper and the HMM on every call's critical path).
  // Returns, for a lane with a bin, the lane's rank among the wave's lanes of the same bin, their number, and whether it leads them.
  auto wave_bins = [&](bool on, uint32_t bin, uint32_t& rank, uint32_t& count, uint32_t& leader) {
    const int lane = tid & 63;
    unsigned long long todo = __ballot(on);
    rank = 0; count = 0; leader = 0;
    while (todo) {
      const int lead = (int)__builtin_ctzll(todo);
      const uint32_t bb = (uint32_t)__builtin_amdgcn_readlane((int)bin, lead);
      const unsigned long long same = __ballot(on && bin == bb);
      if (on && bin == bb) { rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)); count = (uint32_t)__popcll(same); leader = (uint32_t)lead; }
      todo &= ~same;
    }
  };
  const uint32_t n_round = (a.n + 1023u) & ~1023u;  // (whole waves walk the loops: the ballots need every lane)
  for (uint32_t i = (uint32_t)tid; i < n_round; i += 1024) {
    const uint32_t v = i < a.n ? probe(i) : 0u;
    if (i < a.n && i < HMM_RESOLVE_LDS) verdict[i] = v;
    uint32_t rank, count, leader;
    const uint32_t bin = v ? bin_of(v - 1u) : 0u;
    wave_bins(v != 0u, bin, rank, count, leader);
    if (v && rank == 0u) atomicAdd(&hist[bin], count);
  }
  __syncthreads();
  if (tid == 0) { uint32_t run = 0; for (int b = 0; b < 64; ++b) { cursor[b] = run; run += hist[b]; } *a.n_jobs = run; }
  __syncthreads();
  for (uint32_t i = (uint32_t)tid; i < n_round; i += 1024) {
    const uint32_t v = i < a.n ? (i < HMM_RESOLVE_LDS ? verdict[i] : probe(i)) : 0u;
    uint32_t rank, count, leader;
    const uint32_t bin = v ? bin_of(v - 1u) : 0u;
    wave_bins(v != 0u, bin, rank, count, leader);
    uint32_t base = 0;
    if (v && rank == 0u) base = atomicAdd(&cursor[bin], count);
    base = (uint32_t)__shfl((int)base, (int)leader);  // (the first lane of a bin's group holds its base; lanes without a job read lane 0)
    if (!v) continue;
    HmmJobDev jd = a.cand[i];
    jd.seq_len = v - 1u;
    a.jobs[base + rank] = jd;
  }
}

// The same in two launches of many workgroups, all classes of a call at once (round 3: the one-workgroup kernel above took 0.14 ms per
// class -- twenty dependent rounds of probes on one CU -- between the genotyper and the HMM of every call).  First launch: verdict per
// candidate, counts per (class, length bin) through one atomic per wave and key; second launch: every workgroup scans the 8 x 64 counts
// itself (longest bin first within a class) and reserves the places of its candidates, again one atomic per wave and key.
constexpr int HMM_SLOT_CLASSES = 9;         // launch classes of the locus path: 0 .. 7 as in hmm_set_class, 8 = the large models (hmm_viterbi_big_kernel)
constexpr int HMM_PPL_CLASSES = 8;          // classes 0 .. 7 can hold sets with a position-per-lane fill (ppl::PplSegs has a segment for each); the large models behind them cannot
static_assert(HMM_SLOT_CLASSES == HMM_PPL_CLASSES + 1, "the class of the large models follows the classes of hmm_viterbi_kernel");
constexpr int HMM_RESOLVE_KEYS = 64 * HMM_SLOT_CLASSES;  // (class, length bin) counters
struct HmmResolveAllArgs {
  const HmmJobDev* cand; uint32_t n;        // all candidates, classes back to back
  uint32_t class_begin[HMM_SLOT_CLASSES + 1];  // class k = candidates [class_begin[k], class_begin[k + 1])
  const uint8_t* skip_locus; const int32_t* n_alleles; const uint32_t* allele_len;
  HmmJobDev* jobs; uint32_t* n_jobs;        // job list of class k at jobs + class_begin[k], its length at n_jobs[k]
  uint32_t* n_spans; double* purity;
  uint32_t* verdict; uint32_t* hist; uint32_t* taken;  // [n], [HMM_RESOLVE_KEYS], [HMM_RESOLVE_KEYS] (hist and taken cleared by the caller)
  uint32_t len_shift;
  const uint8_t* seq_blob; uint8_t* dup;   // dup [n] (optional): 1 = the second allele of a locus equals the first -- no job, its results are copied (hmm_dup_copy_kernel)
};
__device__ __forceinline__ void hmm_wave_keys(bool on, uint32_t key, int lane, uint32_t& rank, uint32_t& count, uint32_t& leader) {
  unsigned long long todo = __ballot(on);
  rank = 0; count = 0; leader = 0;
  while (todo) {
    const int lead = (int)__builtin_ctzll(todo);
    const uint32_t kk = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
    const unsigned long long same = __ballot(on && key == kk);
    if (on && key == kk) { rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)); count = (uint32_t)__popcll(same); leader = (uint32_t)lead; }
    todo &= ~same;
  }
}
__device__ __forceinline__ uint32_t hmm_class_of(const HmmResolveAllArgs& a, uint32_t i) {
  uint32_t k = 0;
#pragma unroll
  for (int c = 1; c < HMM_SLOT_CLASSES; ++c) k += i >= a.class_begin[c] ? 1u : 0u;
  return k;
}
__global__ void __launch_bounds__(256) hmm_resolve_count_kernel(const HmmResolveAllArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t v = 0, key = 0;
  if (i < a.n) {
    const uint32_t slot = a.cand[i].job_index, l = slot >> 1, al = slot & 1u;
    const bool on = !a.skip_locus[l] && (int32_t)al < a.n_alleles[l];
    if (!on) { a.n_spans[slot] = 0; a.purity[slot] = __builtin_nan(""); }  // what the caller's arrays hold for an allele that is not there
    v = on ? a.allele_len[slot] + 1u : 0u;
    // a homozygous locus labels the same sequence twice in the reference (label_with_hmm per allele, tr.rs:454-492): here the second
    // allele gets no job when it equals the first byte for byte (the candidates of a locus sit next to each other)
    if (a.dup) {
      uint8_t d = 0;
      if (on && al == 1u && i > 0 && a.cand[i - 1].job_index == slot - 1u && a.allele_len[slot - 1u] == a.allele_len[slot]) {
        const uint8_t* p = a.seq_blob + a.cand[i - 1].seq_off; const uint8_t* q = a.seq_blob + a.cand[i].seq_off;
        const uint32_t n = a.allele_len[slot];
        // (eight bases per step, all steps' loads independent of the compare: byte by byte this was 200 dependent loads per thread and
        //  0.18 ms between the genotyper and the HMM of every cfg4 call)
        uint64_t diff = 0;
        uint32_t t = 0;
        for (; t + 8 <= n; t += 8) { uint64_t x, y; __builtin_memcpy(&x, p + t, 8); __builtin_memcpy(&y, q + t, 8); diff |= x ^ y; }
        for (; t < n; ++t) diff |= (uint64_t)(p[t] ^ q[t]);
        d = diff == 0 ? 1 : 0;
      }
      a.dup[i] = d;
      if (d) v = 0;
    }
    a.verdict[i] = v;
    if (v) { const uint32_t b = (v - 1u) >> a.len_shift; key = hmm_class_of(a, i) * 64u + (63u - (b < 63u ? b : 63u)); }
  }
  uint32_t rank, count, leader;
  hmm_wave_keys(v != 0u, key, lane, rank, count, leader);
  if (v && rank == 0u) atomicAdd(&a.hist[key], count);
}
__global__ void __launch_bounds__(256) hmm_resolve_scatter_kernel(const HmmResolveAllArgs a) {
  __shared__ uint32_t base[HMM_RESOLVE_KEYS];
  for (uint32_t t = threadIdx.x; t < (uint32_t)HMM_RESOLVE_KEYS; t += 256) base[t] = a.hist[t];
  __syncthreads();
  if (threadIdx.x < (uint32_t)HMM_SLOT_CLASSES) {  // exclusive scan of a class's bins, bin 0 (the longest alleles) first
    uint32_t run = 0;
    for (int b = 0; b < 64; ++b) { const uint32_t h = base[threadIdx.x * 64 + b]; base[threadIdx.x * 64 + b] = run; run += h; }
    if (blockIdx.x == 0) a.n_jobs[threadIdx.x] = run;
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t v = i < a.n ? a.verdict[i] : 0u;
  uint32_t key = 0, k = 0;
  if (v) { k = hmm_class_of(a, i); const uint32_t b = (v - 1u) >> a.len_shift; key = k * 64u + (63u - (b < 63u ? b : 63u)); }
  uint32_t rank, count, leader;
  hmm_wave_keys(v != 0u, key, lane, rank, count, leader);
  uint32_t at = 0;
  if (v && rank == 0u) at = atomicAdd(&a.taken[key], count);
  at = (uint32_t)__shfl((int)at, (int)leader);
  if (!v) return;
  HmmJobDev jd = a.cand[i];
  jd.seq_len = v - 1u;
  a.jobs[a.class_begin[k] + base[key] + at + rank] = jd;
}

// Behind the HMM kernels: the results of a locus' first allele copied to its second one where hmm_resolve_count_kernel found them equal
__global__ void __launch_bounds__(256) hmm_dup_copy_kernel(const HmmJobDev* __restrict__ cand, uint32_t n, const uint8_t* __restrict__ dup, const HmmSetDev* __restrict__ sets,
                                                           int32_t* __restrict__ spans3, uint32_t* __restrict__ n_spans, uint32_t* __restrict__ counts, double* __restrict__ purity) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !dup[i]) return;
  const HmmJobDev a = cand[i - 1], b = cand[i];
  const uint32_t ns = n_spans[a.job_index];
  n_spans[b.job_index] = ns; purity[b.job_index] = purity[a.job_index];
  for (uint32_t k = 0; k < 3 * ns; ++k) spans3[3 * b.span_off + k] = spans3[3 * a.span_off + k];
  const uint32_t nm = sets[b.set].n_blocks - 1;
  for (uint32_t k = 0; k < nm; ++k) counts[b.count_off + k] = counts[a.count_off + k];
}

// Compaction of the per-job span lists (each job owns a worst-case region) into one dense array for the D2H copy.
__global__ void hmm_pack_spans_kernel(const int32_t* __restrict__ spans3, const uint64_t* __restrict__ job_span_off,
                                      const uint32_t* __restrict__ n_spans, const uint64_t* __restrict__ packed_off,
                                      int32_t* __restrict__ packed, uint64_t n_jobs) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_jobs) return;
  const int32_t* src = spans3 + 3 * job_span_off[j];
  int32_t* dst = packed + 3 * packed_off[j];
  for (uint32_t i = 0; i < 3 * n_spans[j]; ++i) dst[i] = src[i];
}

// exclusive prefix of the span counts (one workgroup): where every job's spans go in the packed array; off[n] = their total
__global__ void __launch_bounds__(1024) hmm_span_prefix_kernel(const uint32_t* __restrict__ n_spans, uint64_t* __restrict__ off, uint64_t n) {
  block_prefix_u32(n_spans, off, n);
}


#include "hmm_batch.hpp"  // the host side of a batch

}  // namespace trgt

using namespace trgt;

// ---- C entry points
extern "C" uint64_t trgt_hmm_path_capacity(uint32_t seq_len, uint32_t max_motif_len) {
  if (seq_len == 0) return 1;
  return (uint64_t)(seq_len + 2) * (max_motif_len + 4) + 8;
}

// Developer / test entry: builds the models of the motif sets both ways -- on the device (what every other entry point uses) and with
// the host builder -- and counts the bytes in which the set descriptors and the table blobs differ (0 expected).
extern "C" int trgt_hmm_models_check(trgt_hip_ctx* c, int32_t n_sets, const uint8_t* motif_blob, const uint32_t* motif_off,
                                     const uint32_t* set_motif_begin, int64_t* n_diff) {
  if (!c || !n_diff) return TRGT_ERR_INVALID;
  *n_diff = -1;
  HmmModels dev, host;
  int rc = hmm_models_on_device(c, n_sets, motif_blob, motif_off, set_motif_begin, dev, c->stream, nullptr);
  if (rc) return fail(c, rc, "%s", dev.err.empty() ? trgt_hip_last_error(c) : dev.err.c_str());
  rc = hmm_build_models(n_sets, motif_blob, motif_off, set_motif_begin, host);
  if (rc) return fail(c, rc, "%s", host.err.c_str());
  std::vector<uint8_t> got((size_t)dev.blob_bytes);
  if (dev.blob_bytes) { const int d2h_rc = trgt::d2h(c, got.data(), dev.d_blob, (size_t)dev.blob_bytes, c->stream); if (d2h_rc) return d2h_rc; }
  TRGT_HIP_TRY(c, trgt::stream_wait(c, c->stream));
  int64_t diff = dev.blob_bytes > host.blob.size() ? (int64_t)(dev.blob_bytes - host.blob.size()) : (int64_t)(host.blob.size() - dev.blob_bytes);
  const size_t n = std::min((size_t)dev.blob_bytes, host.blob.size());
  for (size_t i = 0; i < n; ++i) diff += got[i] != host.blob[i];
  const uint8_t *a = (const uint8_t*)dev.sets.data(), *b = (const uint8_t*)host.sets.data();
  for (size_t i = 0; i < sizeof(HmmSetDev) * (size_t)n_sets; ++i) diff += a[i] != b[i];
  *n_diff = diff;
  return TRGT_OK;
}

extern "C" int trgt_hmm_batch(trgt_hip_ctx* c, int32_t n_sets, const uint8_t* motif_blob, const uint32_t* motif_off,
                              const uint32_t* set_motif_begin, int64_t n_jobs, const uint32_t* job_set,
                              const uint8_t* seq_blob, const uint64_t* seq_off, const uint32_t* seq_len, uint16_t* path,
                              const uint64_t* path_off, uint32_t* path_len, int32_t* spans3, const uint64_t* span_off,
                              uint32_t* n_spans, uint32_t* motif_counts, const uint64_t* count_off, double* purity,
                              int32_t* edit_dist, int32_t* max_dist) {
  HmmBatchIO io;
  io.n_sets = n_sets; io.motif_blob = motif_blob; io.motif_off = motif_off; io.set_motif_begin = set_motif_begin;
  io.n_jobs = n_jobs; io.job_set = job_set; io.seq_blob = seq_blob; io.seq_off = seq_off; io.seq_len = seq_len;
  io.path = path; io.path_off = path_off; io.path_len = path_len; io.spans3 = spans3; io.span_off = span_off; io.n_spans = n_spans;
  io.motif_counts = motif_counts; io.count_off = count_off; io.purity = purity; io.edit_dist = edit_dist; io.max_dist = max_dist;
  return hmm_batch_impl(c, nullptr, io);
}
