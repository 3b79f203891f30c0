// trgt_amd/csrc/hmm_batch.hpp -- the host side of an HMM batch: launch classes and their launcher, the model builders, and the stages
// of one enqueue (HmmPlan, HmmCall) behind hmm_enqueue / hmm_enqueue_slots / hmm_collect (hmm_host.hpp).  Part of hmm.hip's translation
// unit: included there, inside namespace trgt, behind the kernels.
#pragma once

// ---- host side of the long trace-back: room for the chunk maps of a job that may be long, and the launch behind a class's fill kernel
// From how many columns on an allele's trace-back goes to the many-wave kernel: 1 536 in a class of thousands of jobs (every long job
// costs that kernel three launches' worth of chunk maps: the hundreds of 0.5-2 kb VNTR alleles of a catalog step were 27 % slower
// through it), 512 in a small class (a pathogenic catalog: the one lane of the fill kernel chasing 1 500 columns was 1.2 ms of a call).
static inline uint32_t hmm_long_min(uint64_t class_jobs) { return class_jobs <= 256 ? 512u : (uint32_t)HMM_LONG_MIN; }  // (2 048 was too many: the 2 000 VNTR candidates of a cfg4 step, 9.2 -> 10.6 ms)
static inline uint64_t hmm_map_words(uint32_t S, uint64_t max_len, uint32_t long_min) {
  const uint64_t L = max_len + 2;
  if (L < (uint64_t)long_min) return 0;
  const uint64_t n_chunks = (L + HMM_LONG_CHUNK - 1) / HMM_LONG_CHUNK;
  return n_chunks * (3ull * S + 8ull) + 8;
}
static size_t hmm_long_lds_bytes(uint32_t S, uint32_t nb) {
  size_t o = 64 + (size_t)20 * S + (size_t)20 * nb + ((S + 3) & ~3u) + (((size_t)S / 3 + 15) & ~(size_t)15) + 32;
  return ((o + 15) & ~(size_t)15) + (size_t)(HMM_LONG_THREADS / 64) * (HMM_LONG_STG + 512) + HMM_LONG_MAP_LDS;
}
static size_t hmm_lds_bytes(uint32_t S, uint32_t nb) {
  size_t o = 64 + (((size_t)HMM_LDS_PER_STATE * S + 15) & ~(size_t)15) + (((size_t)16 * nb + 15) & ~(size_t)15) + (size_t)hmm_stage_bytes((int)((S + 15) & ~15u));
  o += HMM_CODE_WINDOW + HMM_CODE_PAD + (((size_t)S / 3 + 15) & ~(size_t)15) + 12 * (size_t)HMM_VIS_LDS + 4 * (size_t)nb;
  o += 8 + 8 * 64;  // the steps of a trace-back round (l_rec)
  return o + 64;
}


// Launch class of a motif set: 0 = at most 32 states (two alleles per wave of hmm_viterbi_kernel), w = 1 .. max_waves: its workgroup
// of w waves (a thread per lane), above that HMM_CLASS_BIG: hmm_viterbi_big_kernel (hmm_big.hpp; the lanes tiled over 1 024 threads).
// trgt_hmm_batch launches hmm_viterbi_kernel with up to 16 waves, the locus path (hmm_enqueue_slots) with up to 7.
constexpr uint32_t HMM_BATCH_MAX_WAVES = 16, HMM_SLOT_MAX_WAVES = 7, HMM_CLASS_BIG = 17;
static inline uint32_t hmm_set_class(const HmmSetDev& sd, uint32_t max_waves) {
  if (sd.S <= 32) return 0u;
  const uint32_t w = (std::max(sd.S, sd.n_lanes) + 63) / 64;
  return w <= max_waves ? w : HMM_CLASS_BIG;
}
// One class of large models behind the resolved job list [jobs, jobs + nj) (n_jobs_dev: its length on the device, or null)
static int hmm_launch_big(trgt_hip_ctx* c, hipStream_t ls, uint32_t maxS, uint32_t maxnb, uint32_t nj, const HmmJobDev* d_jobs, const HmmSetDev* d_sets, const uint8_t* d_model,
                          const uint8_t* d_seq, uint8_t* d_bp, uint32_t* d_visits, uint16_t* path, uint32_t* plen, int32_t* spans, uint32_t* nsp, uint32_t* cnt, double* pur,
                          int32_t* edit, int32_t* maxd, const uint32_t* n_jobs_dev) {
  const size_t lds = hmm_big_lds(maxS, maxnb).total;
  if (lds > 160 * 1024) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_hmm_batch: LDS need %zu B", lds);
  if (lds > 64 * 1024) TRGT_HIP_TRY(c, hipFuncSetAttribute((const void*)hmm_viterbi_big_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(hmm_viterbi_big_kernel, dim3(nj), dim3(HMM_BIG_THREADS), lds, ls, d_jobs, d_sets, d_model, d_seq, d_bp, d_visits, path, plen, spans, nsp, cnt, pur, edit, maxd, nj, n_jobs_dev);
  TRGT_HIP_TRY(c, hipGetLastError());
  return TRGT_OK;
}

// The position-per-lane fill (hmm_ppl.hpp) of one class's job list, in front of the class's trace-back launch on the same stream: one
// launch per group width the class's sets need (lanes_mask: bit 0 = 8 lanes, 1 = 16, 2 = 32, 3 = 64); a launch walks the whole list
// and takes the jobs of its width (groups of other widths idle: a wave without a job of its own returns at once).
static int hmm_launch_ppl(trgt_hip_ctx* c, int bset, int class_slot, hipStream_t ls, unsigned lanes_mask, const HmmJobDev* d_jobs, const HmmSetDev* d_sets, const uint8_t* d_model,
                          const uint8_t* d_seq, uint8_t* d_bp, const ppl::PplSegs& segs) {
  if (!segs.begin[segs.n_seg]) return TRGT_OK;
  auto launch = [&](int g, hipStream_t s) {
    const uint32_t nj = segs.end_slot[g] > segs.first_slot[g] ? segs.end_slot[g] - segs.first_slot[g] : 0u;  // job slots this width looks at
    if (!nj) return;
    // (rows of one byte per lane; TRGT_HMM_PPL_WIDE in `make DEV=1` builds: the round-5 rows of one byte per state)
#define TRGT_PPL_LAUNCH(GG, NB)                                                                                                                         \
    do { if (c->knobs.hmm_ppl_wide) hipLaunchKernelGGL((ppl::hmm_fill_ppl_kernel<GG, false>), dim3(NB), dim3(64), 0, s, d_jobs, d_sets, d_model, d_seq, d_bp, segs); \
         else hipLaunchKernelGGL((ppl::hmm_fill_ppl_kernel<GG, true>), dim3(NB), dim3(64), 0, s, d_jobs, d_sets, d_model, d_seq, d_bp, segs); } while (0)
    if (g == 0) TRGT_PPL_LAUNCH(8, (nj + 7) / 8);
    else if (g == 1) TRGT_PPL_LAUNCH(16, (nj + 3) / 4);
    else if (g == 2) TRGT_PPL_LAUNCH(32, (nj + 1) / 2);
    else TRGT_PPL_LAUNCH(64, nj);
#undef TRGT_PPL_LAUNCH
  };
  // the widest groups on the class's own stream; the other widths (disjoint jobs) next to it on side streams forked off that stream and
  // joined back into it: one behind the other they added up their tails (a cfg4 class with 32- and 64-lane sets: 0.53 + 0.47 ms in
  // front of its trace-back)
  const bool side_ok = !c->knobs.hmm_ppl_serial && class_slot >= 0 && class_slot < 4 && (lanes_mask & (lanes_mask - 1u)) != 0u;
  if (!side_ok) {
    for (int g = 3; g >= 0; --g) if (lanes_mask & (1u << g)) launch(g, ls);
    return TRGT_OK;
  }
  hipEvent_t& f = c->hmm_ppl_fork[bset][class_slot];
  if (!f) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&f, hipEventDisableTiming));
  TRGT_HIP_TRY(c, hipEventRecord(f, ls));
  int n_side = 0;
  bool first = true;
  for (int g = 3; g >= 0; --g) {
    if (!(lanes_mask & (1u << g))) continue;
    if (first || n_side >= 3) { launch(g, ls); first = false; continue; }
    hipStream_t& s = c->hmm_ppl_side[bset][class_slot][n_side];
    hipEvent_t& j = c->hmm_ppl_join[bset][class_slot][n_side];
    if (!s) TRGT_HIP_TRY(c, make_side_stream(c, &s));
    if (!j) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&j, hipEventDisableTiming));
    TRGT_HIP_TRY(c, hipStreamWaitEvent(s, f, 0));
    launch(g, s);
    TRGT_HIP_TRY(c, hipEventRecord(j, s));
    ++n_side;
  }
  for (int i = 0; i < n_side; ++i) TRGT_HIP_TRY(c, hipStreamWaitEvent(ls, c->hmm_ppl_join[bset][class_slot][i], 0));
  return TRGT_OK;
}
static inline ppl::PplSegs hmm_ppl_one_segment(uint32_t nj, const uint32_t* n_jobs_dev) { ppl::PplSegs g{}; g.begin[1] = nj; g.n_seg = 1; g.counts = n_jobs_dev; for (int w = 0; w < 4; ++w) { g.first_slot[w] = 0; g.end_slot[w] = nj; } return g; }
static inline unsigned hmm_ppl_bit(const HmmSetDev& sd) { const int g = ppl::lanes_for(sd.ppl_lanes); return g == 8 ? 1u : g == 16 ? 2u : g == 32 ? 4u : g == 64 ? 8u : 0u; }

// ---- the launches of one class (jobs of one workgroup size), for a host-built job list (hmm_enqueue) and a device-resolved one
//      (hmm_enqueue_slots) alike.
// The buffers every kernel of a batch gets:
struct HmmLaunchBufs {
  const HmmSetDev* sets; const uint8_t* model; const uint8_t* seq; uint8_t* bp; uint32_t* visits;
  uint16_t* path; uint32_t* plen; int32_t* spans; uint32_t* nsp; uint32_t* cnt; double* pur; int32_t* edit; int32_t* maxd;
};
struct HmmClassLaunch {
  uint32_t cls;                // hmm_set_class of the class's sets (HMM_CLASS_BIG: hmm_viterbi_big_kernel)
  int ordinal;                 // how many classes of this batch were launched before (0: on the batch's stream, else on a side stream)
  int buffer_set;
  const HmmJobDev* jobs;       // the class's jobs (device) ...
  uint32_t nj;                 // ... how many there are (a device-resolved list: at most) ...
  const uint32_t* n_jobs_dev;  // ... and, for a device-resolved list, where the device counted them (else null)
  uint32_t maxS, maxnb;        // largest model of the class
  uint64_t max_len;            // longest allele the class can have
  unsigned ppl_mask;           // group widths of the class's position-per-lane fills (hmm_ppl_bit)
  bool ppl_launched;           // those fills were launched in front, merged over all classes
  size_t first_job, n_listed;  // where the class's jobs begin in the batch's list, and that list's length (S_HMM_LONG fallback, below)
  int64_t cells;               // for the timer
  unsigned* side_used;         // the batch's side streams in use so far (hmm_join_classes)
  HmmLaunchBufs b;
};
constexpr size_t HMM_LONG_PIECE_PAD = 16;

// The `lds_per_job` word of hmm_viterbi_kernel, as its first lines decode it:
//   bits  0-22  LDS bytes of one job (a multiple of 16)
//   bit   23    the position-per-lane fill wrote rows of one byte per lane (hmm_fill_ppl_kernel<G, true>), not one per state
//   bits 24-29  columns from which an allele goes to hmm_traceback_long_kernel, / 256 (0: HMM_LONG_MIN)
//   bit   30    the back-pointers of sets with ppl_lanes are there already (hmm_fill_ppl_kernel ran in front)
//   bit   31    TRGT_HMM_FOUR_ROUNDS
static uint32_t hmm_viterbi_flags(const trgt_hip_ctx* c, size_t lds_job, unsigned ppl_mask, uint32_t long_min) {
  return (uint32_t)lds_job | (c->knobs.hmm_four_rounds ? 0x80000000u : 0u) | (ppl_mask ? 0x40000000u : 0u) | (ppl_mask && !c->knobs.hmm_ppl_wide ? 0x00800000u : 0u) | ((long_min / 256u) << 24);
}
// The four instantiations of hmm_viterbi_kernel: two alleles per wave or one, score columns in registers (one-wave classes) or in LDS
struct HmmViterbiFn {
  const void* fn;
  void (*launch)(dim3 grid, dim3 block, size_t lds, hipStream_t ls, const HmmClassLaunch& a, uint32_t flags, uint32_t* d_long);
};
template <int SUB, bool ONE_WAVE>
static void hmm_launch_viterbi(dim3 grid, dim3 block, size_t lds, hipStream_t ls, const HmmClassLaunch& a, uint32_t flags, uint32_t* d_long) {
  hipLaunchKernelGGL((hmm_viterbi_kernel<SUB, ONE_WAVE>), grid, block, lds, ls, a.jobs, a.b.sets, a.b.model, a.b.seq, a.b.bp, a.b.visits, a.b.path, a.b.plen, a.b.spans,
                     a.b.nsp, a.b.cnt, a.b.pur, a.b.edit, a.b.maxd, a.nj, flags, a.n_jobs_dev, d_long);
}
template <int SUB, bool ONE_WAVE>
static HmmViterbiFn hmm_viterbi_fn() { return {(const void*)hmm_viterbi_kernel<SUB, ONE_WAVE>, hmm_launch_viterbi<SUB, ONE_WAVE>}; }

// The trace-back of a class 0 whose alleles were all filled in packed rows of 8 / 16 lanes: hmm_trace_ppl_kernel<G>, 64 / G alleles per
// wave; a class with both widths takes hmm_trace_ppl_both_kernel, one launch whose workgroups walk the list once per width (each pass
// skips the other's jobs, as the fills do).
// TRGT_HMM_TRACE_WIDE=1 (developer builds): hmm_viterbi_kernel<32, .> with its fill skipped, two alleles per wave, as before.
static inline bool hmm_trace_packed(const trgt_hip_ctx* c, const HmmClassLaunch& a) {
  return a.cls == 0 && a.ppl_mask != 0 && (a.ppl_mask & ~3u) == 0 && !c->knobs.hmm_ppl_wide && !c->knobs.hmm_no_ppl && !c->knobs.hmm_trace_wide &&
         a.maxS <= (uint32_t)HMM_TP_MAX_STATES && a.maxnb <= (uint32_t)HMM_TP_MAX_BLOCKS;
}
static void hmm_launch_trace_ppl(hipStream_t ls, const HmmClassLaunch& a, uint32_t long_min, uint32_t* d_long) {
  HmmTracePplArgs t{a.jobs, a.b.sets, a.b.model, a.b.seq, (const uint8_t*)a.b.bp, a.b.visits, a.b.path, a.b.plen, a.b.spans, a.b.nsp, a.b.cnt, a.b.pur, a.b.edit, a.b.maxd,
                    a.nj, a.n_jobs_dev, {0u, 0u}, (int)long_min, d_long, 0u};
  t.lds_per_job[0] = (uint32_t)hmm_trace_ppl_lds(8, (int)a.maxS, (int)a.maxnb).total;
  t.lds_per_job[1] = (uint32_t)hmm_trace_ppl_lds(16, (int)a.maxS, (int)a.maxnb).total;
  const uint32_t blocks8 = (a.nj + 7) / 8, blocks16 = (a.nj + 3) / 4;
  const size_t lds8 = 8 * (size_t)t.lds_per_job[0], lds16 = 4 * (size_t)t.lds_per_job[1];
  if ((a.ppl_mask & 3u) == 3u) {
    t.n_blocks8 = blocks8;
    hipLaunchKernelGGL(hmm_trace_ppl_both_kernel, dim3(blocks8 + blocks16), dim3(64), std::max(lds8, lds16), ls, t);
  } else if (a.ppl_mask & 1u) hipLaunchKernelGGL((hmm_trace_ppl_kernel<8>), dim3(blocks8), dim3(64), lds8, ls, t);
  else hipLaunchKernelGGL((hmm_trace_ppl_kernel<16>), dim3(blocks16), dim3(64), lds16, ls, t);
}

// The classes of a batch run next to each other: the first on the batch's stream, the others on side streams forked off it (three per
// buffer set, in rotation) and joined back into it.  A class is bounded by its longest allele: one behind the other they add up their tails.
static int hmm_fork_record(trgt_hip_ctx* c, int buffer_set) {  // where the side streams fork off: in front of the first class's launch
  hipEvent_t& ev = c->hmm_fork[buffer_set ? 1 : 0];
  if (!ev) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  TRGT_HIP_TRY(c, hipEventRecord(ev, c->stream));
  return TRGT_OK;
}
static int hmm_class_stream(trgt_hip_ctx* c, int buffer_set, int ordinal, unsigned& side_used, hipStream_t* ls) {
  *ls = c->stream;
  if (ordinal == 0) return TRGT_OK;
  const int sidx = (ordinal - 1) % 3 + (buffer_set ? 3 : 0);
  if (!c->hmm_side[sidx]) TRGT_HIP_TRY(c, make_side_stream(c, &c->hmm_side[sidx]));
  if (!c->hmm_join[sidx]) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&c->hmm_join[sidx], hipEventDisableTiming));
  *ls = c->hmm_side[sidx];
  TRGT_HIP_TRY(c, hipStreamWaitEvent(*ls, c->hmm_fork[buffer_set ? 1 : 0], 0));
  side_used |= 1u << sidx;
  return TRGT_OK;
}
static int hmm_join_classes(trgt_hip_ctx* c, unsigned side_used) {
  for (int sidx = 0; sidx < 6; ++sidx)
    if (side_used & (1u << sidx)) {
      TRGT_HIP_TRY(c, hipEventRecord(c->hmm_join[sidx], c->hmm_side[sidx]));
      TRGT_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->hmm_join[sidx], 0));
    }
  return TRGT_OK;
}

static int hmm_launch_class(trgt_hip_ctx* c, const HmmClassLaunch& a) {
  int rc;
  const bool half = a.cls == 0;             // two alleles per wave
  const bool big = a.cls == HMM_CLASS_BIG;  // (hmm_viterbi_big_kernel: no position-per-lane fill, its own trace-back for every length)
  const size_t lds_job = big ? 0 : (hmm_lds_bytes(a.maxS, a.maxnb) + 15) & ~(size_t)15;
  const size_t lds = half ? 2 * lds_job : lds_job;
  if (lds > 160 * 1024) return fail(c, TRGT_ERR_UNSUPPORTED, "trgt_hmm_batch: LDS need %zu B", lds);
  const bool regs = !c->knobs.hmm_lds_fill;  // one-wave classes keep the score columns in registers (TRGT_HMM_LDS_FILL=1: in LDS like the others)
  const HmmViterbiFn k = half ? (regs ? hmm_viterbi_fn<32, true>() : hmm_viterbi_fn<32, false>())
                              : (regs && a.cls == 1 ? hmm_viterbi_fn<64, true>() : hmm_viterbi_fn<64, false>());
  if (lds > 64 * 1024) TRGT_HIP_TRY(c, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipStream_t ls;
  if ((rc = hmm_class_stream(c, a.buffer_set, a.ordinal, *a.side_used, &ls))) return rc;
  KTimer t(c, TRGT_K_HMM, ls);
  const HmmLaunchBufs& b = a.b;
  if (big) {
    if ((rc = hmm_launch_big(c, ls, a.maxS, a.maxnb, a.nj, a.jobs, b.sets, b.model, b.seq, b.bp, b.visits, b.path, b.plen, b.spans, b.nsp, b.cnt, b.pur, b.edit, b.maxd, a.n_jobs_dev))) return rc;
    t.stop(a.cells);
    return TRGT_OK;
  }
  // (the class's list of long alleles: filled by the fill kernel, worked off by the trace-back kernel right behind it)
  uint32_t* d_long_cls = nullptr;
  const uint32_t long_min_cls = hmm_long_min(a.nj);
  if (!c->knobs.hmm_no_long_tb && a.max_len + 2 >= (uint64_t)long_min_cls) {
    if (void* z = zero_take(c, ((size_t)a.nj + 16) * 4)) d_long_cls = (uint32_t*)z;  // [count | job indices] of this class, the count cleared
    else {
      // no zero arena: S_HMM_LONG, n_listed + HMM_LONG_PIECE_PAD * (HMM_CLASS_BIG + 1) words.  The class with `ordinal` classes in
      // front of it, whose jobs are [first_job, first_job + nj) of the batch's list, has the nj + HMM_LONG_PIECE_PAD words from
      // first_job + HMM_LONG_PIECE_PAD * ordinal on: the pieces follow each other without overlap, whatever the classes' sizes.
      void* dl = nullptr;
      const int so = a.buffer_set ? (int)S_HMM_B_BASE - (int)S_HMM_SEQ : 0;
      if ((rc = dev_get(c, S_HMM_LONG + so, (a.n_listed + HMM_LONG_PIECE_PAD * (HMM_CLASS_BIG + 1)) * 4, &dl))) return rc;
      d_long_cls = (uint32_t*)dl + a.first_job + HMM_LONG_PIECE_PAD * (size_t)a.ordinal;
      TRGT_HIP_TRY(c, hipMemsetAsync(d_long_cls, 0, 4, ls));
    }
  }
  if (a.ppl_mask && !a.ppl_launched &&
      (rc = hmm_launch_ppl(c, a.buffer_set ? 1 : 0, a.ordinal & 3, ls, a.ppl_mask, a.jobs, b.sets, b.model, b.seq, b.bp, hmm_ppl_one_segment(a.nj, a.n_jobs_dev)))) return rc;
  const bool packed_trace = hmm_trace_packed(c, a);
  if (c->knobs.debug) fprintf(stderr, "[hmm] class %u: %u jobs, trace-back by %s\n", a.cls, a.nj, packed_trace ? "hmm_trace_ppl_kernel" : "hmm_viterbi_kernel");
  if (packed_trace) {
    hmm_launch_trace_ppl(ls, a, long_min_cls, d_long_cls);
  } else k.launch(dim3(half ? (a.nj + 1) / 2 : a.nj), dim3(half ? 64 : 64 * a.cls), lds, ls, a, hmm_viterbi_flags(c, lds_job, a.ppl_mask, long_min_cls), d_long_cls);
  TRGT_HIP_TRY(c, hipGetLastError());
  if (d_long_cls) {
    const size_t llds = hmm_long_lds_bytes(a.maxS, a.maxnb);
    if (llds > 64 * 1024) TRGT_HIP_TRY(c, hipFuncSetAttribute((const void*)hmm_traceback_long_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)llds));
    const int G = c->knobs.hmm_long_wgs;  // workgroups per long allele (1: one launch, the whole trace-back by one workgroup; else the phases 1 / 2 / 3)
    for (int ph = G > 1 ? 1 : 0; ph <= (G > 1 ? 3 : 0); ++ph) {
      const int g = ph == 1 || ph == 3 ? G : 1;
      hipLaunchKernelGGL(hmm_traceback_long_kernel, dim3((unsigned)std::min<uint32_t>(a.nj, 64u) * (unsigned)g), dim3(HMM_LONG_THREADS), llds, ls, a.jobs, b.sets, b.model, b.seq,
                         (const uint8_t*)b.bp, b.visits, b.path, b.plen, b.spans, b.nsp, b.cnt, b.pur, b.edit, b.maxd, (const uint32_t*)d_long_cls,
                         ph | (a.ppl_mask && !c->knobs.hmm_ppl_wide ? 0x100 : 0), g);  // (bit 8: rows of one byte per lane, as bit 23 above)
    }
    TRGT_HIP_TRY(c, hipGetLastError());
  }
  t.stop(a.cells);
  return TRGT_OK;
}

// All motif-set models of a batch (host side).  Thread-safe: touches no ctx state.
int hmm_build_models(int32_t n_sets, const uint8_t* motif_blob, const uint32_t* motif_off, const uint32_t* set_motif_begin, HmmModels& out) {
  char msg[160];
  out.rc = 0;
  std::vector<HmmSetDev>& sets = out.sets;
  sets.assign((size_t)n_sets, HmmSetDev());
  std::vector<std::vector<uint8_t>> blobs((size_t)n_sets);
  std::vector<int> set_err((size_t)n_sets, 0);
  {
    const int nthr = (int)std::min<int64_t>(std::max(1u, std::min(32u, std::thread::hardware_concurrency())), std::max(1, n_sets / 64));
    auto work = [&](int t) {
      for (int s = t; s < n_sets; s += nthr) {
        std::vector<std::string> motifs;
        for (uint32_t m = set_motif_begin[s]; m < set_motif_begin[s + 1]; ++m) {
          std::string mot((const char*)motif_blob + motif_off[m], motif_off[m + 1] - motif_off[m]);
          if (mot.empty()) { set_err[s] = 1; break; }
          static const char allowed[] = "ATCGN";  // replace_invalid_bases(m, ATCGN)
          for (size_t i = 0; i < mot.size(); ++i)
            if (mot[i] == 0 || !std::strchr("ATCGN", mot[i])) mot[i] = allowed[i % 5];
          motifs.push_back(mot);
        }
        if (set_err[s]) continue;
        if (motifs.empty()) { set_err[s] = 2; continue; }
        build_set(motifs, blobs[s], sets[s]);
        if (sets[s].S > HMM_BIG_MAX_STATES || sets[s].n_lanes > HMM_BIG_MAX_STATES) set_err[s] = 3;
        else if (sets[s].n_blocks > 254) set_err[s] = 4;
      }
    };
    if (nthr <= 1) work(0);
    else {
      std::vector<std::thread> th;
      for (int t = 0; t < nthr; ++t) th.emplace_back(work, t);
      for (auto& x : th) x.join();
    }
  }
  std::vector<uint8_t>& blob = out.blob;
  {
    uint64_t total = 0;
    for (int s = 0; s < n_sets; ++s) {
      if (set_err[s] == 1) { snprintf(msg, sizeof msg, "trgt_hmm_batch: empty motif in set %d", s); out.err = msg; return out.rc = TRGT_ERR_INVALID; }
      if (set_err[s] == 2) { snprintf(msg, sizeof msg, "trgt_hmm_batch: set %d has no motif", s); out.err = msg; return out.rc = TRGT_ERR_INVALID; }
      if (set_err[s] == 3) { snprintf(msg, sizeof msg, "trgt_hmm_batch: set %d has %u HMM states on %u lanes (kernel limit %u)", s, sets[s].S, sets[s].n_lanes, HMM_BIG_MAX_STATES); out.err = msg; return out.rc = TRGT_ERR_UNSUPPORTED; }
      if (set_err[s] == 4) { snprintf(msg, sizeof msg, "trgt_hmm_batch: set %d has too many motifs", s); out.err = msg; return out.rc = TRGT_ERR_UNSUPPORTED; }
      total += blobs[s].size();
    }
    blob.resize((size_t)total);
    uint64_t pos = 0;
    for (int s = 0; s < n_sets; ++s) {
      std::memcpy(blob.data() + pos, blobs[s].data(), blobs[s].size());
      HmmSetDev& d = sets[s];
      d.off_inlp += pos; d.off_em += pos; d.off_inst += pos; d.off_block += pos; d.off_nin += pos; d.off_level += pos;
      d.off_flags += pos; d.off_blocks += pos; d.off_motifs += pos; d.off_perm += pos;
      pos += blobs[s].size();
      std::vector<uint8_t>().swap(blobs[s]);
    }
  }
  return 0;
}


// All motif-set models of a batch, built ON THE DEVICE (hmm_model_build_kernel): the host lays the sets out (sizes, offsets, lane
// tables: a few microseconds per thousand sets), uploads the motifs and the logarithm table (kilobytes) and launches one workgroup per
// set -- instead of building ~2 KB of tables per set on host threads and uploading them (6 ms + 22 MB for a 10k-locus batch: it had
// become the critical path of stage C).  Uploads and the kernel go to `up` (a stream with nothing in front of it); `done` is recorded
// behind them.  out.sets / out.d_sets / out.d_blob are valid on return (the device side once `done` has fired).
int hmm_models_on_device(trgt_hip_ctx* c, int32_t n_sets, const uint8_t* motif_blob, const uint32_t* motif_off, const uint32_t* set_motif_begin,
                         HmmModels& out, hipStream_t up, hipEvent_t done) {
  out.rc = 0; out.blob.clear(); out.d_sets = out.d_blob = nullptr;
  std::vector<HmmSetDev>& sets = out.sets;
  sets.assign((size_t)n_sets, HmmSetDev());
  if (n_sets <= 0) return TRGT_OK;
  const uint32_t m_total = set_motif_begin[n_sets];
  const uint32_t byte0 = motif_off[0], bytes_total = motif_off[m_total] - byte0;
  // layout: per set
  std::vector<uint16_t> perm_all, perm;
  std::vector<uint64_t> perm_src((size_t)n_sets, 0);
  std::vector<uint32_t> mlens, blocks, seed_row((size_t)m_total, 0);
  std::vector<double> seed_tab;
  std::vector<int64_t> row_of_len;  // motif length -> first entry of its row (-1: none yet)
  uint64_t pos = 0;
  char msg[160];
  for (int s = 0; s < n_sets; ++s) {
    const uint32_t m0 = set_motif_begin[s], m1 = set_motif_begin[s + 1];
    if (m1 <= m0) { snprintf(msg, sizeof msg, "trgt_hmm_batch: set %d has no motif", s); out.err = msg; return out.rc = TRGT_ERR_INVALID; }
    if (m1 - m0 + 1 > 254) { snprintf(msg, sizeof msg, "trgt_hmm_batch: set %d has too many motifs", s); out.err = msg; return out.rc = TRGT_ERR_UNSUPPORTED; }
    mlens.clear();
    for (uint32_t m = m0; m < m1; ++m) {
      const uint32_t n = motif_off[m + 1] - motif_off[m];
      if (n == 0) { snprintf(msg, sizeof msg, "trgt_hmm_batch: empty motif in set %d", s); out.err = msg; return out.rc = TRGT_ERR_INVALID; }
      mlens.push_back(n);
      if (row_of_len.size() <= n) row_of_len.resize((size_t)n + 1, -1);
      if (row_of_len[n] < 0) {  // ln(seed * (n - k)), k = 1 .. n - 1 (builder.rs:80-173), entry 0 unused
        row_of_len[n] = (int64_t)seed_tab.size();
        const double seed = 2.00 * (1.00 - 0.90) / (double)((size_t)n * (size_t)(n - 1));
        seed_tab.push_back(0.0);
        for (uint32_t k = 1; k < n; ++k) seed_tab.push_back(std::log(seed * (double)(n - k)));
      }
      seed_row[m] = (uint32_t)row_of_len[n];
    }
    HmmSetDev& d = sets[(size_t)s];
    const uint64_t bytes = layout_set(mlens.data(), (uint32_t)mlens.size(), d, blocks, perm);
    if (d.S > HMM_BIG_MAX_STATES || d.n_lanes > HMM_BIG_MAX_STATES) { snprintf(msg, sizeof msg, "trgt_hmm_batch: set %d has %u HMM states on %u lanes (kernel limit %u)", s, d.S, d.n_lanes, HMM_BIG_MAX_STATES); out.err = msg; return out.rc = TRGT_ERR_UNSUPPORTED; }
    d.off_inlp += pos; d.off_em += pos; d.off_inst += pos; d.off_block += pos; d.off_nin += pos; d.off_level += pos;
    d.off_flags += pos; d.off_blocks += pos; d.off_motifs += pos; d.off_perm += pos;
    pos += bytes;
    if (!perm.empty()) { perm_src[(size_t)s] = perm_all.size(); perm_all.insert(perm_all.end(), perm.begin(), perm.end()); }
  }
  out.blob_bytes = pos;
  // one pinned slab -> one device slab: sets | motif_off (rebased) | set_motif_begin | seed_row | perm_src | seed_tab | perm_all | motif bytes
  struct Lay { size_t total = 0; size_t add(size_t b) { const size_t o = total; total += (b + 15) & ~(size_t)15; return o; } } lay;
  const size_t o_sets = lay.add(sizeof(HmmSetDev) * (size_t)n_sets), o_moff = lay.add(4 * ((size_t)m_total + 1)), o_smb = lay.add(4 * ((size_t)n_sets + 1)),
               o_srow = lay.add(4 * (size_t)m_total), o_psrc = lay.add(8 * (size_t)n_sets), o_stab = lay.add(8 * seed_tab.size()),
               o_perm = lay.add(2 * perm_all.size()), o_mot = lay.add(bytes_total);
  void *h = nullptr, *dv = nullptr, *d_blob = nullptr, *d_sets = nullptr;
  int rc;
  if ((rc = pin_get(c, P_HMM_BUILD, lay.total, &h)) || (rc = dev_get(c, S_HMM_BUILD, lay.total, &dv)) ||
      (rc = dev_get(c, S_HMM_MODEL, (size_t)pos + 16, &d_blob)))
    return out.rc = rc;
  uint8_t* hb = (uint8_t*)h;
  std::memcpy(hb + o_sets, sets.data(), sizeof(HmmSetDev) * (size_t)n_sets);
  { uint32_t* q = (uint32_t*)(hb + o_moff); for (uint32_t m = 0; m <= m_total; ++m) q[m] = motif_off[m] - byte0; }
  std::memcpy(hb + o_smb, set_motif_begin, 4 * ((size_t)n_sets + 1));
  std::memcpy(hb + o_srow, seed_row.data(), 4 * (size_t)m_total);
  std::memcpy(hb + o_psrc, perm_src.data(), 8 * (size_t)n_sets);
  std::memcpy(hb + o_stab, seed_tab.data(), 8 * seed_tab.size());
  if (!perm_all.empty()) std::memcpy(hb + o_perm, perm_all.data(), 2 * perm_all.size());
  {  // replace_invalid_bases(m, ATCGN) (utils.rs:29-42), position inside the motif
    uint8_t* q = hb + o_mot;
    static const char allowed[] = "ATCGN";
    for (uint32_t m = 0; m < m_total; ++m) {
      const uint8_t* src = motif_blob + motif_off[m];
      const uint32_t n = motif_off[m + 1] - motif_off[m];
      uint8_t* dst = q + (motif_off[m] - byte0);
      for (uint32_t i = 0; i < n; ++i) { const uint8_t ch = src[i]; dst[i] = (ch == 'A' || ch == 'T' || ch == 'C' || ch == 'G' || ch == 'N') ? ch : (uint8_t)allowed[i % 5]; }
    }
  }
  TRGT_HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = h2d_small(c, dv, h, lay.total, up, -1))) return out.rc = rc;  // (pinned source; a kernel copy: not queued behind bulk uploads)
  // (the descriptors stay where they were uploaded -- the build slab lives as long as the models; the padding between a set's tables is
  //  cleared by the build kernel itself, so that the blob compares equal to the host builder's: a D2D copy and a 20-MB fill per call less)
  d_sets = (uint8_t*)dv + o_sets;
  HmmBuildArgs a;
  const uint8_t* db = (const uint8_t*)dv;
  a.sets = (const HmmSetDev*)(db + o_sets); a.blob = (uint8_t*)d_blob; a.motif_bytes = db + o_mot; a.motif_off = (const uint32_t*)(db + o_moff);
  a.set_motif_begin = (const uint32_t*)(db + o_smb); a.seed_row = (const uint32_t*)(db + o_srow); a.seed_tab = (const double*)(db + o_stab);
  a.perm_all = (const uint16_t*)(db + o_perm); a.perm_src = (const uint64_t*)(db + o_psrc); a.blob_bytes = pos; a.k = hmm_build_consts();
  hipLaunchKernelGGL(hmm_model_build_kernel, dim3((unsigned)n_sets), dim3(64), 0, up, a);
  TRGT_HIP_TRY(c, hipGetLastError());
  if (done) TRGT_HIP_TRY(c, hipEventRecord(done, up));
  out.d_sets = d_sets; out.d_blob = d_blob;
  return TRGT_OK;
}

// State of an enqueued HMM batch between hmm_enqueue / hmm_enqueue_slots (uploads + kernel launches, no host wait for the kernels) and
// hmm_collect (result copies).  One batch per ctx and buffer set may be pending: the device buffers are the ctx's pool slots.
struct HmmPending {
  // ---- both paths
  int64_t n_jobs = 0;            // entries of the per-job results: the jobs of a host-built list, the slots (two per locus) of a device-resolved one
  hipStream_t stream = nullptr;  // the stream the batch was enqueued on
  int32_t* spans3 = nullptr; const uint64_t* span_off = nullptr;  // the caller's spans and their layout ...
  bool spans_on_host = false;    // ... in host memory: they come back packed.  The packed copy is made behind the kernels at enqueue time
  const int32_t* d_packed = nullptr; const uint64_t* d_poff = nullptr; uint64_t packed_cap_bytes = 0;  // (HmmCall::pack): collect only copies
  uint32_t* cnt_user = nullptr; uint64_t cnt_total = 0;        // motif counts in a host array go back job by job (result_buffers):
  std::vector<uint64_t> cnt_off; std::vector<uint32_t> cnt_n;  // the jobs' ranges (a host-built list: known at enqueue time; else hmm_slots_resolved)
  DevOut<uint16_t> o_path; DevOut<uint32_t> o_plen, o_nsp, o_cnt; DevOut<int32_t> o_spans, o_edit, o_maxd; DevOut<double> o_pur;
  // ---- a host-built list (hmm_enqueue)
  std::vector<uint64_t> tight_off;  // the jobs' spans in the tight device layout: source of the pack tables' upload, so it lives as long as the batch
  // ---- a device-resolved list (hmm_enqueue_slots): what hmm_slots_resolved needs of every slot once the genotyper is back
  std::vector<uint32_t> slot_nm;    // motifs of the slot's set
  std::vector<uint64_t> slot_cnt_off;
};

void hmm_pending_free(HmmPending* p) { delete p; }

// Behind the kernels of a batch whose spans go to host memory: prefix of the span counts + compaction of the per-job span lists into
// the back-pointer workspace (free once the kernels are through; at least 16 B per (base, state-row) >= 12 B per possible span).
// hmm_collect then copies counts, total and the first HMM_PACKED_FIRST bytes of the packed spans in ONE go -- the host used to wait for
// the counts, build the offsets, upload them, launch the compaction and wait again (0.5 ms of a 10k-locus call's tail).
constexpr size_t HMM_PACKED_FIRST = 1u << 20;

// ---- the plan of a batch (host only).  hmm_enqueue and hmm_enqueue_slots fill it -- HmmCall::plan_host_list, HmmCall::plan_slots: they
//      differ in where a job's columns come from and in how the list is ordered -- and every later stage reads it.
struct HmmClassPlan {            // one launch class: jobs [begin, begin + count) of the list as it is uploaded
  uint32_t begin = 0, count = 0;
  uint32_t maxS = 0, maxnb = 0;  // largest model
  uint64_t max_len = 0;          // longest allele the class can have
  unsigned ppl_mask = 0;         // group widths of its position-per-lane fills (hmm_ppl_bit)
};
struct HmmPlan {
  HmmClassPlan cls[HMM_CLASS_BIG + 1];  // by hmm_set_class (a batch has few of them); the classes are listed and launched in this order
  uint64_t bp_total = 0, visit_total = 0;                    // workspace: bytes of back-pointers, words of visits and chunk maps
  uint64_t path_total = 0, span_total = 0, count_total = 0;  // extents of the caller's layouts
  uint64_t span_dev_bytes = 0;                               // not 0: the spans have a device buffer of their own, in a tight layout: copied back packed, or not at all
  int64_t cells = 0;                                         // for the timer (of a device-resolved list hmm_slots_resolved counts them)
  const bool no_long_tb, no_ppl;                             // the knobs a plan depends on
  explicit HmmPlan(const trgt_hip_ctx* c) : no_long_tb(c->knobs.hmm_no_long_tb), no_ppl(c->knobs.hmm_no_ppl) {}

  void set_begins() { uint32_t at = 0; for (HmmClassPlan& q : cls) { q.begin = at; at += q.count; } }  // once every job is counted
  uint32_t n_listed() const { return cls[HMM_CLASS_BIG].begin + cls[HMM_CLASS_BIG].count; }
  // a job of `columns` bases of set `sd` joins class k (its count is taken separately: the layout below needs it before the first job is placed)
  void join_class(uint32_t k, const HmmSetDev& sd, uint64_t columns) {
    HmmClassPlan& q = cls[k];
    q.maxS = std::max(q.maxS, sd.S); q.maxnb = std::max(q.maxnb, sd.n_blocks); q.max_len = std::max(q.max_len, columns);
    if (!no_ppl && k != HMM_CLASS_BIG) q.ppl_mask |= hmm_ppl_bit(sd);  // (hmm_viterbi_big_kernel has no such fill)
  }
  // One job's piece of the back-pointer / visit / chunk-map workspace: a model of S states over `columns` bases (the allele of a
  // host-built list; the longest allele the locus can have for a slot, whose allele the device only finds later), in class k of
  // `class_jobs` jobs.  Pieces follow each other in the order of the calls.
  void place(HmmJobDev& jd, uint32_t S, uint64_t columns, uint32_t k, uint64_t class_jobs) {
    const uint64_t spad = (S + 15) & ~15u;
    // Invariant (hmm_ppl.hpp): every job's rows start 16 bytes into its piece -- bytes [bp_off - 16, bp_off) take the stores of roles a lane of the
    // position-per-lane fill does not have, and a wave's lanes without a job store to bytes 0..15 of the workspace through the fake
    // bp_off = 16; no row of any job may ever start below 16 (tests/test_hmm_gpu.py compares both fills on long alleles)
    jd.bp_off = bp_total + 16; bp_total += 16 + align_up(spad * (columns + 2), 16);
    jd.visit_off = visit_total; visit_total += 3ull * (columns + 2);
    const uint64_t mw = no_long_tb || k == HMM_CLASS_BIG ? 0 : hmm_map_words(S, columns, hmm_long_min(class_jobs));  // chunk maps of a job that may be long
    jd.map_off = mw ? visit_total + 4 : 0; visit_total += mw ? mw + 4 : 0;
  }
  int check_workspace(trgt_hip_ctx* c) const {
    return bp_total > c->ws_limit ? fail(c, TRGT_ERR_NOMEM, "trgt_hmm_batch: back-pointer workspace %llu B exceeds limit", (unsigned long long)bp_total) : TRGT_OK;
  }
};
// The locus path numbers its classes 0 .. HMM_SLOT_CLASSES - 1 (the device counts the jobs of each): the classes of hmm_viterbi_kernel
// keep their numbers, the large models come right behind them.
static inline uint32_t hmm_slot_class(uint32_t k) { return k == HMM_CLASS_BIG ? (uint32_t)HMM_SLOT_CLASSES - 1 : k; }
static_assert(HMM_SLOT_MAX_WAVES == HMM_PPL_CLASSES - 1, "classes 0 .. HMM_SLOT_MAX_WAVES of the locus path, then the large models");

// The order of a host-built list: by class (stable; usually there is one class, and nothing to sort), and inside a class the longest
// alleles first: workgroups start in list order, and a launch ends with its last allele -- a 10-kb allele started behind a thousand
// short ones is pure tail.  (Classes of many alleles of similar length -- the single STR motif of a whole-genome catalog -- are left
// alone: sorting twenty thousand jobs costs more than it saves.)
template <class ClassOf>
static void hmm_order_host_list(std::vector<HmmJobDev>& jobs, ClassOf job_class) {
  bool mixed = false;
  const uint32_t c0 = job_class(jobs[0]);
  for (const auto& jd : jobs) if (job_class(jd) != c0) { mixed = true; break; }
  if (mixed) std::stable_sort(jobs.begin(), jobs.end(), [&](const HmmJobDev& a, const HmmJobDev& b) { return job_class(a) < job_class(b); });
  size_t b0 = 0;
  while (b0 < jobs.size()) {
    size_t b1 = b0; uint32_t mx = 0; uint64_t sum = 0;
    const uint32_t jc = job_class(jobs[b0]);
    while (b1 < jobs.size() && job_class(jobs[b1]) == jc) { mx = std::max(mx, jobs[b1].seq_len); sum += jobs[b1].seq_len; ++b1; }
    const size_t n = b1 - b0;
    if (n > 1 && (n <= 4096 || (uint64_t)mx * n > 4 * sum))
      std::stable_sort(jobs.begin() + (ptrdiff_t)b0, jobs.begin() + (ptrdiff_t)b1, [](const HmmJobDev& a, const HmmJobDev& b) { return a.seq_len > b.seq_len; });
    b0 = b1;
  }
}

// ---- one enqueue.  hmm_enqueue and hmm_enqueue_slots (below) run its stages in order; what a stage leaves for a later one is a member.
//      Every HIP call, and every zero_take (pieces of one arena: their order fixes addresses), is issued in the order of those lists.
struct HmmCall {
  trgt_hip_ctx* const c; const int buffer_set, so;  // so: slot offset of the buffer set
  std::unique_ptr<HmmPending> P;
  HmmModels local_models; const HmmModels* mp = nullptr;  // the batch's models: the caller's, or built here
  HmmPlan plan;
  std::vector<HmmJobDev> jobs;           // a host-built list, in upload order
  HmmJobDev* h_jobs = nullptr;           // the list (a device-resolved one: its candidates) in pinned memory
  const uint64_t* pack_off = nullptr;    // where a job's spans are on the device, for the packing behind the kernels
  const void *d_sets = nullptr, *d_model = nullptr; const uint8_t* d_seq = nullptr;
  void *d_jobs = nullptr, *d_bp = nullptr, *d_visits = nullptr, *d_pack_tabs = nullptr;
  // a device-resolved list: candidates | resolved list | counts per class ... | verdicts (pieces of d_jobs, or of the zero arena)
  HmmJobDev *d_cand = nullptr, *d_list = nullptr; uint32_t *d_count = nullptr, *d_verdict = nullptr; bool count_cleared = false;
  const uint8_t* d_dup = nullptr; bool ppl_merged = false;
  // (S_HMM_JOBS of a device-resolved list: candidates | job lists | counts per class (16 words) | 2 x HMM_RESOLVE_KEYS resolve counters | verdicts)
  static constexpr size_t count_bytes = 64 + 8 * (size_t)HMM_RESOLVE_KEYS;

  HmmCall(trgt_hip_ctx* c_, int buffer_set_) : c(c_), buffer_set(buffer_set_), so(buffer_set_ ? (int)S_HMM_B_BASE - (int)S_HMM_SEQ : 0), plan(c_) {}
  size_t list_bytes() const { return (size_t)plan.n_listed() * sizeof(HmmJobDev); }
  // where class k of the locus path (hmm_slot_class) begins in a device-resolved list; k = HMM_SLOT_CLASSES: where the list ends
  uint32_t slot_class_begin(int k) const { return k < HMM_PPL_CLASSES ? plan.cls[k].begin : k < HMM_SLOT_CLASSES ? plan.cls[HMM_CLASS_BIG].begin : plan.n_listed(); }
  HmmLaunchBufs bufs() const {
    return HmmLaunchBufs{(const HmmSetDev*)d_sets, (const uint8_t*)d_model, d_seq, (uint8_t*)d_bp, (uint32_t*)d_visits, P->o_path.dev, P->o_plen.dev,
                         P->o_spans.dev, P->o_nsp.dev, P->o_cnt.dev, P->o_pur.dev, P->o_edit.dev, P->o_maxd.dev};
  }

  // ---- stages of both paths
  int begin(int64_t n_results, const HmmBatchIO& io) {  // the device, and the pending state
    TRGT_HIP_TRY(c, hipSetDevice(c->device));
    P.reset(new HmmPending());
    P->n_jobs = n_results; P->spans3 = io.spans3; P->span_off = io.span_off; P->stream = c->stream;
    return TRGT_OK;
  }
  int workspace(size_t jobs_bytes) {
    int rc;
    if ((rc = dev_get(c, S_HMM_JOBS + so, jobs_bytes, &d_jobs)) || (rc = dev_get(c, S_HMM_BP + so, (size_t)plan.bp_total, &d_bp)) ||
        (rc = dev_get(c, S_HMM_VISITS + so, (size_t)plan.visit_total * 4, &d_visits)))
      return rc;
    return TRGT_OK;
  }
  // The list goes up once, from pinned memory (a pageable source makes the "async" copy a blocking staged one).  With it, BEFORE the
  // kernels are enqueued, the offsets of the per-job span lists for pack() -- on the copy stream in the slots path -- and not behind the
  // kernels on the batch's stream, where that upload sat on the critical path of every call's tail (round 5).
  // d_pack_tabs: packed offsets [n + 1] (written by pack) | the jobs' offsets [n]
  int upload_jobs(hipStream_t us) {
    int rc;
    const int64_t n = P->n_jobs;
    if ((rc = h2d_small(c, d_jobs, h_jobs, list_bytes(), us, -1))) return rc;
    if (P->spans_on_host && ((rc = dev_get(c, S_HMM_MOTIFS + so, (size_t)n * 16 + 16, &d_pack_tabs)) ||
                             (rc = h2d_small(c, (uint64_t*)d_pack_tabs + (n + 1), pack_off, (size_t)n * 8, us, S_HMM_MOTIFS + so))))
      return rc;
    if (us != c->stream) {
      if (!c->ev_upload) TRGT_HIP_TRY(c, hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming));
      TRGT_HIP_TRY(c, hipEventRecord(c->ev_upload, us));
      TRGT_HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_upload, 0));
    }
    return TRGT_OK;
  }
  // The eight result buffers.  An output the caller does not ask for (a null pointer) gets none, a device array is written in place, a
  // host array gets a pool slot that hmm_collect copies back.
  int result_buffers(const HmmBatchIO& io) {
    int rc;
    HmmPending& p = *P;
    const size_t n = (size_t)p.n_jobs;
    if ((rc = p.o_path.init(c, S_HMM_PATH + so, io.path, (size_t)plan.path_total)) || (rc = p.o_plen.init(c, S_HMM_PLEN + so, io.path_len, n))) return rc;
    // Spans: when the caller's buffer is host memory the kernel writes a tight per-job layout on the device and only the
    // spans actually produced are copied back (packed); a device buffer is written in the caller's layout directly.
    // spans3 == NULL: the caller only wants purity / counts (filter_impure_trs); the spans stay in the tight device layout
    if (plan.span_dev_bytes) {
      void* d = nullptr;
      if ((rc = dev_get(c, S_HMM_SPANS + so, (size_t)plan.span_dev_bytes, &d))) return rc;
      p.o_spans.user = io.spans3; p.o_spans.dev = (int32_t*)d; p.o_spans.count = 0; p.o_spans.staged = false;  // copied back packed (hmm_collect)
    } else if ((rc = p.o_spans.init(c, S_HMM_SPANS + so, io.spans3, (size_t)plan.span_total * 3))) return rc;
    if ((rc = p.o_nsp.init(c, S_HMM_NSP + so, io.n_spans, n)) || (rc = p.o_cnt.init(c, S_HMM_CNT + so, io.motif_counts, (size_t)plan.count_total))) return rc;
    if (p.o_cnt.staged) {  // host array shared with other batches: only the ranges of this batch's jobs may be written back (hmm_collect)
      p.cnt_user = io.motif_counts; p.cnt_total = plan.count_total; p.o_cnt.staged = false;
    }
    if ((rc = p.o_pur.init(c, S_HMM_PUR + so, io.purity, n)) || (rc = p.o_edit.init(c, S_HMM_EDIT + so, io.edit_dist, n)) ||
        (rc = p.o_maxd.init(c, S_HMM_MAXD + so, io.max_dist, n)))
      return rc;
    return TRGT_OK;
  }
  // One launch per class; the first on the batch's stream, the others on side streams forked off it, so that the classes run next to
  // each other (a class is bounded by its longest allele: one behind the other they add up their tails).
  // The fork event sits behind the uploads (the resolve kernel and the merged fills of a device-resolved list) and IN FRONT of the first
  // launch: recorded behind it (as it was until the cfg3 trace showed it), every other class waited for the first class to finish --
  // 17.6 + 15.2 ms instead of 17.6 for the 10-kb alleles of cfg3.
  // list: the jobs on the device; counts: where the device counted the jobs of every hmm_slot_class (a device-resolved list), else null.
  int launch_classes(const HmmJobDev* list, const uint32_t* counts) {
    int rc;
    if ((rc = hmm_fork_record(c, buffer_set))) return rc;
    HmmClassLaunch cl{};
    cl.buffer_set = buffer_set; cl.n_listed = plan.n_listed(); cl.ppl_launched = ppl_merged; cl.b = bufs();
    unsigned side_used = 0;
    cl.side_used = &side_used;
    for (uint32_t k = 0; k <= HMM_CLASS_BIG; ++k) {
      const HmmClassPlan& q = plan.cls[k];
      if (!q.count) continue;
      cl.cls = k; cl.maxS = q.maxS; cl.maxnb = q.maxnb; cl.max_len = q.max_len; cl.ppl_mask = q.ppl_mask;
      cl.jobs = list + q.begin; cl.nj = q.count; cl.first_job = q.begin; cl.n_jobs_dev = counts ? counts + hmm_slot_class(k) : nullptr;
      cl.cells = cl.ordinal == 0 ? plan.cells : 0;
      if ((rc = hmm_launch_class(c, cl))) return rc;
      ++cl.ordinal;
    }
    return hmm_join_classes(c, side_used);
  }
  // the compaction behind the kernels (HMM_PACKED_FIRST, above)
  int pack() {
    if (!P->spans_on_host) return TRGT_OK;
    const int64_t n = P->n_jobs;
    uint64_t* d_poff = (uint64_t*)d_pack_tabs; const uint64_t* d_toff = d_poff + (n + 1);
    hipLaunchKernelGGL(hmm_span_prefix_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t*)P->o_nsp.dev, d_poff, (uint64_t)n);
    hipLaunchKernelGGL(hmm_pack_spans_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const int32_t*)P->o_spans.dev, d_toff, (const uint32_t*)P->o_nsp.dev,
                       (const uint64_t*)d_poff, (int32_t*)d_bp, (uint64_t)n);
    TRGT_HIP_TRY(c, hipGetLastError());
    P->d_packed = (const int32_t*)d_bp; P->d_poff = d_poff; P->packed_cap_bytes = plan.bp_total;
    return TRGT_OK;
  }

  // ---- a host-built list
  int check_list(const HmmBatchIO& io) {
    if (io.n_sets < 0 || io.n_jobs < 0 || (io.n_jobs > 0 && (!io.motif_blob || !io.motif_off || !io.set_motif_begin || !io.job_set || !io.seq_off ||
                                                              !io.seq_len || (io.spans3 && !io.span_off) || !io.n_spans || !io.motif_counts ||
                                                              !io.count_off || !io.purity)))
      return fail(c, TRGT_ERR_INVALID, "trgt_hmm_batch: null argument");
    if (io.path && !io.path_off) return fail(c, TRGT_ERR_INVALID, "trgt_hmm_batch: path without path_off");
    return TRGT_OK;
  }
  // models (built on the device: hmm_model_build_kernel): built here unless the caller prepared them ahead of time (trgt_locus_batch
  // does, concurrently with the flank-location stage)
  int models(const HmmModels* premade, const HmmBatchIO& io) {
    mp = premade;
    if (!mp) {
      const int mrc = hmm_models_on_device(c, io.n_sets, io.motif_blob, io.motif_off, io.set_motif_begin, local_models, c->stream, nullptr);
      if (mrc) return fail(c, mrc, "%s", local_models.err.empty() ? trgt_hip_last_error(c) : local_models.err.c_str());
      mp = &local_models;
    } else if (mp->rc) return fail(c, mp->rc, "%s", mp->err.c_str());
    return TRGT_OK;
  }
  // Jobs in the caller's order -- a job's columns are its allele's bases, and its piece of the workspace follows the job's before it in
  // THAT order --, then sorted: by class up to HMM_BATCH_MAX_WAVES, longest first (hmm_order_host_list).
  int plan_host_list(const HmmBatchIO& io) {
    const std::vector<HmmSetDev>& sets = mp->sets;
    const int64_t n_jobs = io.n_jobs;
    auto set_class = [&](uint32_t s) { return hmm_set_class(sets[s], HMM_BATCH_MAX_WAVES); };
    for (int64_t j = 0; j < n_jobs; ++j) {
      if ((int32_t)io.job_set[j] >= io.n_sets) return fail(c, TRGT_ERR_INVALID, "trgt_hmm_batch: job %lld bad set", (long long)j);
      plan.cls[set_class(io.job_set[j])].count += 1;
    }
    plan.set_begins();
    // spans3 in host memory, or none: the tight layout (result_buffers)
    const bool tight = io.spans3 == nullptr || !is_device_ptr(io.spans3);
    P->spans_on_host = tight && io.spans3 != nullptr;
    if (tight) P->tight_off.resize((size_t)n_jobs);
    uint64_t tight_total = 0;
    jobs.resize((size_t)n_jobs);
    for (int64_t j = 0; j < n_jobs; ++j) {
      const HmmSetDev& sd = sets[io.job_set[j]];
      const uint32_t k = set_class(io.job_set[j]), len = io.seq_len[j];
      HmmJobDev& jd = jobs[(size_t)j];
      jd.set = io.job_set[j]; jd.seq_len = len; jd.job_index = (uint32_t)j;
      jd.seq_off = io.seq_off[j]; jd.span_off = io.spans3 ? io.span_off[j] : 0; jd.count_off = io.count_off[j];
      jd.path_off = io.path ? io.path_off[j] : 0;
      jd.path_cap = (uint32_t)std::min<uint64_t>(trgt_hmm_path_capacity(len, sd.max_mlen), 0xFFFFFFFFull);
      plan.place(jd, sd.S, len, k, plan.cls[k].count);
      plan.join_class(k, sd, len);
      if (tight) { jd.span_off = P->tight_off[(size_t)j] = tight_total; tight_total += (uint64_t)len + 1; }
      else plan.span_total = std::max<uint64_t>(plan.span_total, io.span_off[j] + len + 1);
      plan.count_total = std::max<uint64_t>(plan.count_total, io.count_off[j] + (sd.n_blocks - 1));
      P->cnt_off.push_back(io.count_off[j]); P->cnt_n.push_back(sd.n_blocks - 1);
      if (io.path) plan.path_total = std::max<uint64_t>(plan.path_total, io.path_off[j] + jd.path_cap);
      plan.cells += (int64_t)sd.S * ((int64_t)len + 2);
    }
    plan.span_dev_bytes = tight_total * 12;  // (0 for a device array: every job has a triple, so a tight layout is never empty)
    pack_off = P->tight_off.data();
    if (int rc = plan.check_workspace(c)) return rc;
    hmm_order_host_list(jobs, [&](const HmmJobDev& j) { return set_class(j.set); });
    return TRGT_OK;
  }
  // the alleles: a device blob as it is; host sequences go up packed (the caller's blob is usually sparse: one max-length slot per allele)
  int sequences(const HmmBatchIO& io) {
    if (is_device_ptr(io.seq_blob)) { d_seq = io.seq_blob; return TRGT_OK; }
    int rc;
    const int64_t n_jobs = io.n_jobs;
    uint64_t tight = 0;
    for (int64_t j = 0; j < n_jobs; ++j) tight += io.seq_len[j];
    void *h_tight = nullptr, *d_tight = nullptr;
    if ((rc = pin_get(c, buffer_set ? P_HMM_SEQ_B : P_HMM_SEQ, (size_t)tight + 16, &h_tight)) || (rc = dev_get(c, S_HMM_SEQ + so, (size_t)tight + 16, &d_tight))) return rc;
    std::vector<uint64_t> toff((size_t)n_jobs);
    uint64_t o = 0;
    for (int64_t j = 0; j < n_jobs; ++j) { toff[(size_t)j] = o; std::memcpy((uint8_t*)h_tight + o, io.seq_blob + io.seq_off[j], io.seq_len[j]); o += io.seq_len[j]; }
    for (auto& jd : jobs) jd.seq_off = toff[jd.job_index];
    if ((rc = h2d_small(c, d_tight, h_tight, (size_t)tight, c->stream, -1))) return rc;
    d_seq = (const uint8_t*)d_tight;
    return TRGT_OK;
  }
  // the model tables: where the device builder left them, or (models of the host builder) uploaded here
  int model_tables() {
    if (mp->d_sets && mp->d_blob) { d_sets = mp->d_sets; d_model = mp->d_blob; return TRGT_OK; }
    int rc;
    void *ds = nullptr, *dm = nullptr;
    if ((rc = dev_get(c, S_HMM_DESC, mp->sets.size() * sizeof(HmmSetDev), &ds))) return rc;
    if ((rc = dev_get(c, S_HMM_MODEL, mp->blob.size(), &dm))) return rc;
    TRGT_HIP_TRY(c, hipMemcpyAsync(ds, mp->sets.data(), mp->sets.size() * sizeof(HmmSetDev), hipMemcpyHostToDevice, c->stream));
    TRGT_HIP_TRY(c, hipMemcpyAsync(dm, mp->blob.data(), mp->blob.size(), hipMemcpyHostToDevice, c->stream));
    d_sets = ds; d_model = dm;
    return TRGT_OK;
  }
  int pin_job_list() {
    void* h = nullptr;
    if (int rc = pin_get(c, buffer_set ? P_HMM_JOBS_B : P_HMM_JOBS, list_bytes(), &h)) return rc;
    std::memcpy(h, jobs.data(), list_bytes());
    h_jobs = (HmmJobDev*)h;
    return TRGT_OK;
  }

  // ---- stage C behind a device-side genotyper: the kernels are enqueued before the host knows which alleles exist (see
  //      hmm_resolve_kernel); hmm_slots_resolved tells the pending batch afterwards, hmm_collect is the same as for a host-built list.
  int check_slots(const HmmSlots& in, const HmmBatchIO& io) {
    if (!mp->d_sets || !mp->d_blob) return fail(c, TRGT_ERR_INVALID, "hmm_enqueue_slots: the models must be in device memory");
    if (!is_device_ptr(in.seq_blob_dev) || (io.spans3 && is_device_ptr(io.spans3))) return fail(c, TRGT_ERR_INVALID, "hmm_enqueue_slots: device alleles, host results");
    d_sets = mp->d_sets; d_model = mp->d_blob; d_seq = in.seq_blob_dev;
    return TRGT_OK;
  }
  // Two candidates per locus the host does not keep for itself: a slot's columns are the longest allele its locus can have (cap: the
  // device finds the allele later), and its piece of the workspace follows in locus order.  The list is ordered by class up to
  // HMM_SLOT_MAX_WAVES with a counting sort: loci keep their order inside a class.  The candidates are written where they go up from.
  int plan_slots(const HmmSlots& in, const HmmBatchIO& io) {
    const std::vector<HmmSetDev>& sets = mp->sets;
    const int64_t nl = in.n_loci, n_slots = 2 * nl;
    auto set_class = [&](int64_t l) { return hmm_set_class(sets[(size_t)l], HMM_SLOT_MAX_WAVES); };
    for (int64_t l = 0; l < nl; ++l) {
      if (in.host_skip && in.host_skip[l]) continue;
      plan.cls[set_class(l)].count += 2;
    }
    plan.set_begins();
    P->slot_nm.assign((size_t)n_slots, 0); P->slot_cnt_off.assign(io.count_off, io.count_off + n_slots);
    P->spans_on_host = io.spans3 != nullptr;
    for (int64_t sl = 0; sl < n_slots; ++sl) {
      const HmmSetDev& sd = sets[(size_t)(sl >> 1)];
      P->slot_nm[(size_t)sl] = sd.n_blocks - 1;
      plan.count_total = std::max<uint64_t>(plan.count_total, io.count_off[sl] + (sd.n_blocks - 1));
      plan.span_total = std::max<uint64_t>(plan.span_total, io.span_off[sl] + in.cap[sl >> 1] + 1);
    }
    plan.span_dev_bytes = plan.span_total * 12 + 16;  // (in the caller's layout: as tight as it gets before the alleles are known)
    pack_off = io.span_off;
    tl_mark(c, "hmm slots: counted");
    if (plan.n_listed() == 0) return TRGT_OK;
    void* h = nullptr;
    if (int rc = pin_get(c, buffer_set ? P_HMM_JOBS_B : P_HMM_JOBS, list_bytes(), &h)) return rc;
    h_jobs = (HmmJobDev*)h;
    uint32_t at[HMM_CLASS_BIG + 1];
    for (uint32_t k = 0; k <= HMM_CLASS_BIG; ++k) at[k] = plan.cls[k].begin;
    for (int64_t l = 0; l < nl; ++l) {
      if (in.host_skip && in.host_skip[l]) continue;
      const HmmSetDev& sd = sets[(size_t)l];
      const uint32_t k = set_class(l);
      plan.join_class(k, sd, in.cap[l]);
      for (int a = 0; a < 2; ++a) {
        HmmJobDev& jd = h_jobs[at[k]++];
        const int64_t sl = 2 * l + a;
        jd.set = (uint32_t)l; jd.seq_len = 0; jd.job_index = (uint32_t)sl; jd.path_cap = 0;
        jd.seq_off = in.seq_off[sl]; jd.path_off = 0; jd.span_off = io.span_off[sl]; jd.count_off = io.count_off[sl];
        plan.place(jd, sd.S, in.cap[l], k, plan.cls[k].count);  // room for the longest allele the locus can have (+ the dump slot of hmm_fill_ppl_kernel)
      }
    }
    tl_mark(c, "hmm slots: candidates");
    return plan.check_workspace(c);
  }
  // counts | histogram | places taken (cleared): a piece of the call's zero arena when there is one
  void resolve_buffers() {
    const uint32_t n_cand = plan.n_listed();
    d_cand = (HmmJobDev*)d_jobs; d_list = d_cand + n_cand;
    void* const z_count = zero_take(c, count_bytes);
    count_cleared = z_count != nullptr;
    d_count = z_count ? (uint32_t*)z_count : (uint32_t*)((uint8_t*)d_jobs + 2 * list_bytes());
    d_verdict = (uint32_t*)((uint8_t*)d_jobs + 2 * list_bytes() + count_bytes);
  }
  // the job list, resolved on the device from the genotyper's results
  int resolve(const HmmSlots& in) {
    const int64_t nl = in.n_loci, n_slots = 2 * nl;
    const uint32_t n_cand = plan.n_listed();
    HmmPending& p = *P;
    uint32_t max_cap = 1, len_shift = 0;
    for (int64_t l = 0; l < nl; ++l) max_cap = std::max(max_cap, in.cap[l]);
    while ((max_cap >> len_shift) >= 64) ++len_shift;
    // slots that are no candidates at all (loci left to the host path) hold "no allele" too
    if (void* z = p.o_nsp.staged && (size_t)n_slots * 4 <= (512u << 10) ? zero_take(c, (size_t)n_slots * 4) : nullptr) p.o_nsp.dev = (uint32_t*)z;
    else TRGT_HIP_TRY(c, hipMemsetAsync(p.o_nsp.dev, 0, (size_t)n_slots * 4, c->stream));
    if (c->knobs.hmm_resolve_one_wg) {
      for (uint32_t k = 0; k <= HMM_CLASS_BIG; ++k) {
        const HmmClassPlan& q = plan.cls[k];
        if (!q.count) continue;
        HmmResolveArgs ra{d_cand + q.begin, q.count, in.d_skip, in.d_n_alleles, in.d_allele_len, d_list + q.begin, d_count + hmm_slot_class(k), p.o_nsp.dev, p.o_pur.dev, len_shift};
        hipLaunchKernelGGL(hmm_resolve_kernel, dim3(1), dim3(1024), 0, c->stream, ra);
      }
    } else {
      HmmResolveAllArgs ra;
      ra.cand = d_cand; ra.n = n_cand;
      for (int k = 0; k <= HMM_SLOT_CLASSES; ++k) ra.class_begin[k] = slot_class_begin(k);
      ra.skip_locus = in.d_skip; ra.n_alleles = in.d_n_alleles; ra.allele_len = in.d_allele_len;
      ra.jobs = d_list; ra.n_jobs = d_count; ra.n_spans = p.o_nsp.dev; ra.purity = p.o_pur.dev;
      ra.hist = d_count + 16; ra.taken = ra.hist + HMM_RESOLVE_KEYS; ra.verdict = d_verdict; ra.len_shift = len_shift;
      ra.seq_blob = in.seq_blob_dev; ra.dup = c->knobs.hmm_no_dedupe ? nullptr : reinterpret_cast<uint8_t*>(ra.verdict + n_cand);
      d_dup = ra.dup;
      if (!count_cleared) TRGT_HIP_TRY(c, hipMemsetAsync(d_count, 0, count_bytes, c->stream));
      const dim3 rg((unsigned)((n_cand + 255) / 256));
      hipLaunchKernelGGL(hmm_resolve_count_kernel, rg, dim3(256), 0, c->stream, ra);
      hipLaunchKernelGGL(hmm_resolve_scatter_kernel, rg, dim3(256), 0, c->stream, ra);
    }
    TRGT_HIP_TRY(c, hipGetLastError());
    return TRGT_OK;
  }
  // The position-per-lane fills of ALL classes: one launch per group width over the whole list (a segment per class), the widths next
  // to each other (hmm_launch_ppl), the classes' trace-backs behind them.  Per class -- up to four launches on as many streams for
  // each of up to four classes -- the stage had more streams than HIP has hardware queues, and what shares a queue runs one after
  // the other: in a cfg4 trace the second 64-lane fill began 0.7 ms after the stage did (1.47 ms for the stage; 0.57 + 0.3 are its
  // longest fill and trace-back).  TRGT_HMM_PPL_PER_CLASS=1: as before.
  int merged_fills() {
    unsigned all_ppl_mask = 0;
    for (int k = 0; k < HMM_PPL_CLASSES; ++k) all_ppl_mask |= plan.cls[k].ppl_mask;
    ppl_merged = all_ppl_mask != 0 && !c->knobs.hmm_ppl_per_class;
    if (!ppl_merged) return TRGT_OK;
    ppl::PplSegs segs{};
    static_assert(sizeof(segs.begin) / sizeof(segs.begin[0]) == HMM_PPL_CLASSES + 1, "a segment per class that can have such a fill");
    for (int k = 0; k <= HMM_PPL_CLASSES; ++k) segs.begin[k] = slot_class_begin(k);  // (the large models behind them have no such fill)
    segs.n_seg = HMM_PPL_CLASSES; segs.counts = (const uint32_t*)d_count;
    // a width's launch spans the classes that hold sets of that width, not the whole list: a workgroup that finds no job of its width
    // ends at once, but 17 000 of them in front of 3 000 that work made the 64-lane launch of cfg4 0.73 ms instead of 0.54
    for (int w = 0; w < 4; ++w) {
      segs.first_slot[w] = segs.end_slot[w] = 0;
      bool any = false;
      for (int k = 0; k < HMM_PPL_CLASSES; ++k)
        if (plan.cls[k].ppl_mask & (1u << w)) { if (!any) segs.first_slot[w] = segs.begin[k]; segs.end_slot[w] = segs.begin[k + 1]; any = true; }
    }
    KTimer tf(c, TRGT_K_HMM, c->stream);
    if (int rc = hmm_launch_ppl(c, buffer_set ? 1 : 0, 0, c->stream, all_ppl_mask, (const HmmJobDev*)d_list, (const HmmSetDev*)d_sets, (const uint8_t*)d_model, d_seq, (uint8_t*)d_bp, segs)) return rc;
    TRGT_HIP_TRY(c, hipGetLastError());
    tf.stop(0);
    return TRGT_OK;
  }
  // homozygous loci: the second allele's results are the first one's
  int dedupe_copy() {
    if (!d_dup) return TRGT_OK;
    const uint32_t n_cand = plan.n_listed();
    hipLaunchKernelGGL(hmm_dup_copy_kernel, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, c->stream, (const HmmJobDev*)d_cand, n_cand, d_dup, (const HmmSetDev*)d_sets,
                       P->o_spans.dev, P->o_nsp.dev, P->o_cnt.dev, P->o_pur.dev);
    TRGT_HIP_TRY(c, hipGetLastError());
    return TRGT_OK;
  }
};

int hmm_batch_impl(trgt_hip_ctx* c, const HmmModels* premade, const HmmBatchIO& io) {
  HmmPending* pend = nullptr;
  int rc = hmm_enqueue(c, premade, io, &pend);
  if (rc) return rc;
  return hmm_collect(c, pend);
}

int hmm_enqueue(trgt_hip_ctx* c, const HmmModels* premade, const HmmBatchIO& io, HmmPending** out_pending, int buffer_set) {
  *out_pending = nullptr;
  if (!c) return TRGT_ERR_INVALID;
  HmmCall h(c, buffer_set);
  int rc;
  if ((rc = h.check_list(io)) || io.n_jobs == 0) return rc;
  if ((rc = h.begin(io.n_jobs, io)) ||
      (rc = h.models(premade, io)) ||
      (rc = h.plan_host_list(io)) ||
      (rc = h.sequences(io)) ||
      (rc = h.model_tables()) ||
      (rc = h.workspace(h.list_bytes())) ||
      (rc = h.pin_job_list()) ||
      (rc = h.upload_jobs(c->stream)) ||
      (rc = h.result_buffers(io)) ||
      (rc = h.launch_classes((const HmmJobDev*)h.d_jobs, nullptr)) ||
      (rc = h.pack()))
    return rc;
  *out_pending = h.P.release();
  return TRGT_OK;
}

int hmm_enqueue_slots(trgt_hip_ctx* c, const HmmModels* models, const HmmSlots& in, const HmmBatchIO& io, HmmPending** out_pending, int buffer_set) {
  *out_pending = nullptr;
  if (!c) return TRGT_ERR_INVALID;
  if (!models || models->rc) return fail(c, models ? models->rc : TRGT_ERR_INVALID, "%s", models ? models->err.c_str() : "no models");
  if (in.n_loci <= 0) return TRGT_OK;
  HmmCall h(c, buffer_set);
  h.mp = models;
  int rc;
  if ((rc = h.check_slots(in, io)) ||
      (rc = h.begin(2 * in.n_loci, io)) ||
      (rc = h.plan_slots(in, io)))
    return rc;
  if (h.plan.n_listed() == 0) return TRGT_OK;  // every locus is left to the host path
  // (S_HMM_JOBS: candidates | job lists | counts ... | verdicts | duplicates)
  if ((rc = h.workspace(2 * h.list_bytes() + HmmCall::count_bytes + 4 * (size_t)h.plan.n_listed() + (size_t)h.plan.n_listed() + 16))) return rc;
  h.resolve_buffers();
  // the uploads on the copy stream: a copy queued on the batch's stream would sit in the copy engine's queue until the genotyper in
  // front of it has run, and hold up every copy issued after it (the next batch's reads)
  if ((rc = h.upload_jobs(c->stream_copy ? c->stream_copy : c->stream)) ||
      (rc = h.result_buffers(io)) ||
      (rc = h.resolve(in)))
    return rc;
  tl_mark(c, "hmm slots: resolve launched");
  if ((rc = h.merged_fills()) ||
      (rc = h.launch_classes(h.d_list, h.d_count)) ||  // (cells: counted when the genotyper's results are known, hmm_slots_resolved)
      (rc = h.dedupe_copy()))
    return rc;
  tl_mark(c, "hmm slots: classes launched");
  if ((rc = h.pack())) return rc;
  *out_pending = h.P.release();
  return TRGT_OK;
}

int64_t hmm_slots_resolved(trgt_hip_ctx* c, HmmPending* P, const HmmModels* mp, const uint8_t* skip, const int32_t* n_alleles, const uint32_t* allele_len) {
  if (!P) return 0;
  int64_t jobs = 0, cells = 0;
  P->cnt_off.clear(); P->cnt_n.clear();
  for (int64_t sl = 0; sl < P->n_jobs; ++sl) {
    const int64_t l = sl >> 1;
    if (skip[l] || (int32_t)(sl & 1) >= n_alleles[l]) continue;
    P->cnt_off.push_back(P->slot_cnt_off[(size_t)sl]); P->cnt_n.push_back(P->slot_nm[(size_t)sl]);
    cells += (int64_t)mp->sets[(size_t)l].S * ((int64_t)allele_len[sl] + 2);
    ++jobs;
  }
  if (c->timing) c->k_cells[TRGT_K_HMM] += cells;
  return jobs;
}

int hmm_collect(trgt_hip_ctx* c, HmmPending* pend) {
  if (!pend) return TRGT_OK;  // an empty batch
  std::unique_ptr<HmmPending> P(pend);
  struct StreamSwap { trgt_hip_ctx* c; hipStream_t saved; ~StreamSwap() { c->stream = saved; } } stream_swap{c, c->stream};
  c->stream = P->stream;
  const int64_t n_jobs = P->n_jobs;
  const bool spans_on_host = P->spans_on_host;
  int32_t* spans3 = P->spans3; const uint64_t* span_off = P->span_off;
  auto &o_path = P->o_path; auto &o_plen = P->o_plen, &o_nsp = P->o_nsp, &o_cnt = P->o_cnt; auto &o_spans = P->o_spans, &o_edit = P->o_edit, &o_maxd = P->o_maxd; auto& o_pur = P->o_pur;
  int rc;
  const bool tl_on = c->knobs.timeline;
  const auto tl0 = std::chrono::steady_clock::now();
  auto HTL = [&](const char* name, double mb) { if (tl_on) fprintf(stderr, "[tl]   hmm collect %-22s +%6.2f ms  (%.2f MB)\n", name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count(), mb); };
  if (spans_on_host) {
    // counts, total and the head of the packed spans in one round trip (the compaction ran behind the kernels: HmmCall::pack)
    std::vector<uint32_t> h_nsp((size_t)n_jobs);
    uint64_t ptotal = 0;
    const size_t first = (size_t)std::min<uint64_t>(HMM_PACKED_FIRST, P->packed_cap_bytes);
    std::vector<int32_t> h_packed(first / 4 + 4);
    { const int d2h_rc = d2h(c, h_nsp.data(), o_nsp.dev, (size_t)n_jobs * 4, c->stream); if (d2h_rc) return d2h_rc; }
    { const int d2h_rc = d2h(c, &ptotal, P->d_poff + n_jobs, 8, c->stream); if (d2h_rc) return d2h_rc; }
    { const int d2h_rc = d2h(c, h_packed.data(), P->d_packed, first, c->stream); if (d2h_rc) return d2h_rc; }
    TRGT_HIP_TRY(c, stream_wait(c, c->stream));
    HTL("counts + packed spans on host", (double)((size_t)n_jobs * 4 + first) / 1e6);
    if (ptotal * 12 > P->packed_cap_bytes) return fail(c, TRGT_ERR_INVALID, "trgt_hmm_batch: %llu spans do not fit the packing workspace", (unsigned long long)ptotal);
    if (ptotal * 12 > first) {  // the rest (many spans: long alleles of interrupted repeats)
      h_packed.resize((size_t)ptotal * 3 + 4);
      { const int d2h_rc = d2h(c, (uint8_t*)h_packed.data() + first, (const uint8_t*)P->d_packed + first, (size_t)ptotal * 12 - first, c->stream); if (d2h_rc) return d2h_rc; }
      TRGT_HIP_TRY(c, stream_wait(c, c->stream));
      HTL("rest of the packed spans", (double)(ptotal * 12 - first) / 1e6);
    }
    uint64_t at = 0;
    for (int64_t j = 0; j < n_jobs; ++j) {
      std::memcpy(spans3 + 3 * span_off[j], h_packed.data() + 3 * at, (size_t)h_nsp[(size_t)j] * 12);
      at += h_nsp[(size_t)j];
    }
  }
  std::vector<uint32_t> h_cnt;
  if (P->cnt_user && P->cnt_total) {
    h_cnt.resize((size_t)P->cnt_total);
    { const int d2h_rc = d2h(c, h_cnt.data(), o_cnt.dev, (size_t)P->cnt_total * 4, c->stream); if (d2h_rc) return d2h_rc; }
  }
  if ((rc = o_path.finish(c)) || (rc = o_plen.finish(c)) || (rc = o_spans.finish(c)) || (rc = o_nsp.finish(c)) ||
      (rc = o_cnt.finish(c)) || (rc = o_pur.finish(c)) || (rc = o_edit.finish(c)) || (rc = o_maxd.finish(c)))
    return rc;
  HTL("copies enqueued", (double)((o_path.staged ? o_path.count * 2 : 0) + (o_plen.staged ? o_plen.count * 4 : 0) + (o_spans.staged ? o_spans.count * 4 : 0) + (o_nsp.staged ? o_nsp.count * 4 : 0) +
                                  (o_cnt.staged ? o_cnt.count * 4 : 0) + (o_pur.staged ? o_pur.count * 8 : 0) + (o_edit.staged ? o_edit.count * 4 : 0) + (o_maxd.staged ? o_maxd.count * 4 : 0)) / 1e6);
  TRGT_HIP_TRY(c, stream_wait(c, c->stream));
  HTL("synced", 0.0);
#ifdef TRGT_HMM_PROF
  {
    unsigned long long h[16], z[16] = {0};
    TRGT_HIP_TRY(c, hipMemcpyFromSymbol(h, HIP_SYMBOL(g_hmm_prof), sizeof h));
    TRGT_HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_hmm_prof), z, sizeof h));
    const double t = (double)(h[0] + h[1] + h[2] + h[3]) + 1e-9;
    fprintf(stderr, "[hmm prof] jobs=%lld | setup %.1f%% fill %.1f%% traceback %.1f%% path+decode %.1f%% | kcycles/job %.1f\n", (long long)n_jobs,
            100 * h[0] / t, 100 * h[1] / t, 100 * h[2] / t, 100 * h[3] / t, t / 1e3 / (double)n_jobs);
    const double f = (double)(h[8] + h[9] + h[10] + h[11] + h[12] + h[13]) + 1e-9;
    fprintf(stderr, "[hmm prof]   long trace-back (kcycles of thread 0 over all alleles): chunk maps %.0f, stringing %.0f, re-walk %.0f, path order + visits %.0f\n", h[4] / 1e3, h[5] / 1e3, h[6] / 1e3, h[7] / 1e3);
    fprintf(stderr, "[hmm prof]   fill (%.0f kcycles on the profiled lanes): symbol %.1f%% emitting+sync %.1f%% chains+ends+sync %.1f%% run end+sync %.1f%% block starts+sync %.1f%% store %.1f%%\n",
            f / 1e3, 100 * h[8] / f, 100 * h[9] / f, 100 * h[10] / f, 100 * h[11] / f, 100 * h[12] / f, 100 * h[13] / f);
  }
#endif
  if (!h_cnt.empty())
    for (size_t j = 0; j < P->cnt_off.size(); ++j)
      std::memcpy(P->cnt_user + P->cnt_off[j], h_cnt.data() + P->cnt_off[j], (size_t)P->cnt_n[j] * 4);
  return TRGT_OK;
}
