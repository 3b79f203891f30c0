/* trgt_hip_plot.h -- the plot path: what `trgt plot` computes per locus before it draws (src/trvz/), as one batch call.
 *
 *   mode 0, allele plot   get_allele_align (trvz/align_allele.rs:7-14): align_consensus (trvz/align_consensus.rs:9-31) of an allele
 *                         consensus, then align_reads (trvz/align_reads.rs:7-28) of its reads: one end-to-end gap-affine alignment
 *                         with back-trace per read, convert (:31-113), project_betas (trvz/read.rs:24-66), the sort of :26.
 *   mode 1, waterfall     the sort and longest_read of plot_waterfall (trvz/waterfall_plot.rs:28-37) and align (:42-123) of every
 *                         read: two flank alignments, align_motifs (trvz/align_consensus.rs:35-122) of the read's repeat part, the
 *                         padding segment, the three-part split of the betas.
 *
 * Part of include/trgt_hip.h, which includes this file inside its extern "C" block; not meant to be included on its own.
 * Additions to ABI 11.  Rendering (crates/pipeplot), colours, scales, reading the VCF / BAM (trvz/input.rs) and the --max-allele-reads
 * subsampling stay with the caller.
 *
 * A panel is one (locus, allele) in mode 0 and one locus in mode 1.  Panel p owns reads [panel_read_begin[p], panel_read_begin[p + 1]).
 *
 * Segments.  An AlignSeg (trvz/align.rs:11-32) is two uint32_t: width, then op | seg_type << 8.
 *   op        0 Match, 1 Subst, 2 Ins, 3 Del (AlignOp, align.rs:18-24)
 *   seg_type  the motif index for Tr(i); the number of motifs of the panel's set for the unsegmented Tr(motifs.len());
 *             TRGT_PLOT_SEG_LEFT_FLANK (0xFFFE); TRGT_PLOT_SEG_RIGHT_FLANK (0xFFFF)
 * Slot offsets (pseg_off, rseg_off) count segments, not words.
 *
 * Capacity.  A slot must hold trgt_plot_seg_capacity(mode, ref_len, read_len) segments:
 *   mode 0, a read    2 * ref_len + read_len + 3.  convert emits one segment per run of equal (operation, seg type) pairs.  The
 *                     alignment has at most ref_len + read_len operations, so at most as many runs of equal operations; a run is
 *                     cut further only where the seg type of the consensus changes under it, and the consensus has fewer than
 *                     ref_len such changes: fewer than 2 * ref_len + read_len segments.
 *   mode 0, a panel   pass the panel's ref_len and read_len 0.  With t = ref_len - lf_len - rf_len bases in the repeat, align_motifs
 *                     merges neighbours of equal (op, seg type).  Every segment that covers bases covers at least one: at most t of
 *                     them.  A width-0 Ins segment takes the type of the base behind it, and two such segments with no base between
 *                     them share that base and merge: at most t + 1.  With the two flank segments: 2 t + 3 <= 2 * ref_len + 3.
 *   mode 1, a read    2 * max(read_len, ref_len) + 2, where ref_len = lf_len + rf_len.  The two flank alignments have at most
 *                     2 lf_len and 2 rf_len operations, the repeat part of t = read_len - ref_len bases gives at most 2 t + 1
 *                     segments (above), and there is one padding segment: 2 ref_len + 2 t + 2 = 2 read_len + 2.
 *
 * Bytes.  trvz hands sequences and motifs to the HMM without replace_invalid_bases, and what the reference does with other bytes
 * there is pinned by nothing: reads and references must be over ACGT, motifs over ACGTN.
 *
 * Errors.  Every check runs before the first launch and before any output is written; the message names the first offender.
 * TRGT_ERR_INVALID: a NULL among the required arrays; mode not 0 or 1; panel_set out of range; panel_read_begin decreasing;
 * ref_len < lf_len + rf_len (mode 1: !=); a mode-1 read shorter than lf_len + rf_len; a byte outside the alphabets; beta_pos of a read
 * not strictly increasing or >= read_len; in mode 0 an empty consensus (convert indexes seg_type_by_ref[ref_pos - 1] of an empty
 * vector there) and an empty read (no reference test aligns against an empty text).  TRGT_ERR_UNSUPPORTED: a read or consensus beyond
 * the aligner's 2^27 bases per alignment; a motif set beyond the HMM's 4096 states / 253 motifs (worded as
 * trgt_hmm_batch words it); behind the kernels, an alignment whose status is not TRGT_WF_COMPLETED (the message names the read; the
 * outputs are then undefined). */
#ifndef TRGT_HIP_PLOT_H
#define TRGT_HIP_PLOT_H
#ifndef TRGT_HIP_H
#error "include trgt_hip.h, which includes this file"
#endif

#define TRGT_PLOT_SEG_LEFT_FLANK 0xFFFEu
#define TRGT_PLOT_SEG_RIGHT_FLANK 0xFFFFu

typedef struct trgt_plot_in {
  int32_t mode;                        /* 0 allele plot, 1 waterfall */
  int32_t n_sets;                      /* motif sets, exactly as trgt_hmm_batch takes them (host) */
  const uint8_t* motif_blob; const uint32_t* motif_off; const uint32_t* set_motif_begin;
  int64_t n_panels;
  const uint32_t* panel_set;           /* [n_panels] motif set of the panel's locus */
  const uint8_t* ref_blob;             /* host or device.  mode 0: the allele consensus, left flank + allele + right flank (what
                                          get_allele_seqs builds); mode 1: left flank + right flank only */
  const uint64_t* ref_off; const uint32_t* ref_len; const uint32_t* lf_len; const uint32_t* rf_len;   /* [n_panels] */
  const uint64_t* panel_read_begin;    /* [n_panels + 1], starts at 0 */
  const uint8_t* read_blob;            /* host or device, one byte per base */
  const uint64_t* read_off; const uint32_t* read_len;   /* [n_reads] */
  const uint64_t* beta_begin;          /* [n_reads + 1] or NULL (no betas): read r owns beta_pos[beta_begin[r] .. beta_begin[r + 1]) */
  const uint32_t* beta_pos;            /* Beta::pos (trvz/read.rs:15-19), strictly increasing inside a read.  The values stay with the caller */
} trgt_plot_in;

typedef struct trgt_plot_out {         /* every array host or device; optional ones may be NULL.  Of pseg / rseg in host memory only the used
                                          part of every slot is written (the rest of a slot keeps what it held); in HBM a slot is scratch up to its capacity */
  uint32_t* pseg; const uint64_t* pseg_off; uint32_t* n_pseg;   /* mode 0: AlleleAlign::seq of panel p at pseg[2 * pseg_off[p] ..], n_pseg[p] segments.  mode 1: unused, may be NULL */
  uint32_t* rseg; const uint64_t* rseg_off; uint32_t* n_rseg;   /* the Align of read r at rseg[2 * rseg_off[r] ..], n_rseg[r] segments */
  int32_t* beta_proj;                  /* optional, parallel to beta_pos: the projected position; -1: project_betas drops the beta or never reaches it */
  int32_t* score;                      /* optional [n_reads].  mode 0: WfaAlign::score; mode 1: INT32_MIN */
  uint32_t* order;                     /* optional [n_reads]: slot panel_read_begin[p] + k holds the read drawn k-th in panel p -- mode 0: the stable sort
                                          by (read_len, Reverse(score)) of align_reads.rs:26; mode 1: the stable sort by read_len of waterfall_plot.rs:28-31 */
} trgt_plot_out;

/* The aligner is WFAligner::builder(Alignment, MemoryHigh).affine(2, 5, 1).build(): the builder sets no heuristic, so the attribute
 * default WFadaptive(10, 50, 1) stays.  Pattern = the consensus (mode 1: a flank), text = the read (mode 1: its first lf_len and last
 * rf_len bases), end to end. */
int trgt_plot_align_batch(trgt_hip_ctx* ctx, const trgt_plot_in* in, trgt_plot_out* out);
uint64_t trgt_plot_seg_capacity(int32_t mode, uint32_t ref_len, uint32_t read_len);
/* Device time (ms) of plot_motif_segs_kernel and plot_read_segs_kernel in the context's last trgt_plot_align_batch; both 0 unless
 * trgt_hip_timing_enable was on for that call.  cf. trgt_locus_meth_kernel_ms */
int trgt_plot_kernel_ms(const trgt_hip_ctx* ctx, double out[2]);
#endif
