/* trgt_hip_merge.h -- the merge path: what `trgt merge` computes per site between reading N records and writing one, merge_exact
 * (src/merge/strategy/exact.rs:6-88), as one batch call over many sites:
 *
 *   - the set of all ALT sequences of all entries, de-duplicated by their bytes;
 *   - that set ordered by (length, bytes), behind the one REF;
 *   - every GT index rewritten into the new list.
 *
 * Part of include/trgt_hip.h, which includes this file inside its extern "C" block; not meant to be included on its own.  Additions to
 * ABI 11.  The heap over positions, the padding of pre-1.0 files and the FORMAT concatenation of process_format_fields
 * (vcf_processor.rs) are trgt_merge_sites_batch (trgt_hip_merge_sites.h), which leaves a ready trgt_merge_in; reading the VCFs, header
 * merging, the FORMAT strings themselves, skip_n / process_n and writing stay with the caller.
 *
 * Input.  An ENTRY is one input VCF's record at a site; an entry with zero alleles stands for a file that has no record there
 * (process_missing_record).  Site s owns entries [site_entry_begin[s], site_entry_begin[s + 1]); entry e owns alleles
 * [entry_allele_begin[e], entry_allele_begin[e + 1]), the first of which is its REF, and genotype values
 * [entry_gt_begin[e], entry_gt_begin[e + 1]).  The three begin arrays start at 0 and never decrease.  Allele a is the allele_len[a] bytes at
 * allele_blob + allele_off[a]; zero-length alleles are legal, alleles may overlap or share bytes.  Sample boundaries inside an entry do
 * not matter to merge_exact and are not passed.
 *
 * gt is in BCF encoding, as GenotypeAllele converts it: (i + 1) << 1 is Unphased(i), ((i + 1) << 1) | 1 is Phased(i), 0 and 1 are
 * UnphasedMissing and PhasedMissing, TRGT_MERGE_GT_VECTOR_END (INT32_MIN + 1, bcf_int32_vector_end) is passed through untouched, so that
 * the padded arrays of flatten_genotypes can be handed in as they are.
 *
 * Output, per site s, with slot = out_allele_begin[s]:
 *   site_status[s]     0, or the first error of the reference in the reference's order:
 *                        1  "Reference alleles do not match" (exact.rs:16-23): out_allele_src[slot] and [slot + 1] hold the input
 *                           indices of the two REF alleles the message names (the first non-empty entry's and the first that differs);
 *                        2  "No reference allele found" (:32): every entry is empty, or the site has no entries;
 *                        3  a GT index at or beyond its entry's allele count (:61-69).
 *                      A status never fails the call (the reference returns Err per site; merge_variants skips or quits).
 *   out_n_alleles[s]   1 + the number of distinct ALT sequences; 0 for a site with a status.
 *   out_allele_src     [slot .. slot + out_n_alleles[s]): in output order, the index of an input allele that carries the sequence.  [slot]
 *                      is the REF of the site's first non-empty entry; every ALT is the LOWEST input index among its equals.  Bytes are
 *                      not copied: the caller has the blob.
 *   allele_map[a]      the merged index of input allele a.
 *   gt_out[g]          gt[g] with the index replaced, phase bit kept, missing values and vector end unchanged.
 * For a site with a status its part of allele_map / gt_out is unspecified.  A slot is scratch up to its capacity: what lies beyond
 * out_n_alleles[s] (status 1: beyond the two indices) is unspecified.
 *
 * A slot must hold 1 + the number of ALT alleles of the site's entries (before de-duplication), and 2 when the site has two or more
 * non-empty entries (status 1 writes two indices).
 *
 * REF equal to an ALT.  The reference builds its index map by sorted_alleles.iter().enumerate()...collect::<HashMap>() (:41-45): a
 * later equal key overwrites an earlier one.  So when some ALT has the bytes of the REF, the output list keeps BOTH, and every input
 * allele with those bytes -- each entry's REF included, hence GT index 0 -- maps to the ALT's position, not to 0.  This follows from the
 * code and is pinned by neither test of the reference (:94-229); it is reproduced here as it stands.
 *
 * Order.  ALTs are ordered by length, then by unsigned byte comparison (a.cmp(b) on &[u8]): by the first differing BYTE.
 *
 * Errors.  Every check runs before the first launch and before any output is written; the message (trgt_hip_last_error) names the
 * first offender.  TRGT_ERR_INVALID: a NULL among the arrays that have elements (the three begin arrays and out_allele_begin always
 * have); n_sites < 0; a begin array that does not start at 0 or decreases; allele_off + allele_len > blob_len; a negative gt other than
 * vector end; a slot smaller than its site needs.  TRGT_ERR_UNSUPPORTED: 2^31 - 16 or more alleles or genotype values in one call.
 * trgt_merge_exact_host has no context: it returns the same codes and leaves the message where trgt_hip_last_error(NULL) reads it
 * (the library's one context-free error string, shared with trgt_hip_create; not thread-safe).
 *
 * Size.  The device takes sites of up to trgt_merge_site_alleles_limit() input alleles (what its LDS layout holds).  Larger sites are
 * done by the host twin inside the same call, with the same results, and counted in trgt_merge_stats: no site fails a call for size. */
#ifndef TRGT_HIP_MERGE_H
#define TRGT_HIP_MERGE_H
#ifndef TRGT_HIP_H
#error "include trgt_hip.h, which includes this file"
#endif

#define TRGT_MERGE_GT_VECTOR_END (-2147483647)   /* INT32_MIN + 1 */
#define TRGT_MERGE_REF_MISMATCH 1
#define TRGT_MERGE_NO_REF 2
#define TRGT_MERGE_GT_OUT_OF_RANGE 3

typedef struct trgt_merge_in {
  int64_t n_sites;
  const uint64_t* site_entry_begin;     /* [n_sites + 1], host */
  const uint64_t* entry_allele_begin;   /* [n_entries + 1], host */
  const uint64_t* allele_off;           /* [n_alleles], host */
  const uint32_t* allele_len;           /* [n_alleles], host */
  const uint8_t* allele_blob;           /* host or device (trgt_merge_exact_host: host) */
  uint64_t blob_len;
  const uint64_t* entry_gt_begin;       /* [n_entries + 1], host */
  const int32_t* gt;                    /* [n_gt], host */
} trgt_merge_in;

typedef struct trgt_merge_out {         /* every array host or device (trgt_merge_exact_host: host), except out_allele_begin */
  int32_t* site_status;                 /* [n_sites] */
  int32_t* out_n_alleles;               /* [n_sites] */
  int32_t* out_allele_src;              /* [out_allele_begin[n_sites]] */
  const uint64_t* out_allele_begin;     /* [n_sites + 1], host, given by the caller, never decreasing */
  int32_t* allele_map;                  /* [n_alleles] */
  int32_t* gt_out;                      /* [n_gt] */
} trgt_merge_out;

/* merge_hash_kernel and merge_site_kernel (csrc/merge_exact.hip), one workgroup per site; synchronous on the context's stream */
int trgt_merge_exact_batch(trgt_hip_ctx* ctx, const trgt_merge_in* in, trgt_merge_out* out);
/* The host twin: the same results by a sort on one thread.  No context, no GPU, host pointers only */
int trgt_merge_exact_host(const trgt_merge_in* in, trgt_merge_out* out);
/* The compiled ceiling of input alleles per site on the device (no GPU needed) */
int32_t trgt_merge_site_alleles_limit(void);
/* Of the context's last trgt_merge_exact_batch: sites on the device, sites done by the host twin, sites with a status != 0, byte
 * comparisons that went to HBM (two sequences compared in the blob because length and hash, or length and prefix key, agreed) */
int trgt_merge_stats(const trgt_hip_ctx* ctx, int64_t out[4]);
/* Device time (ms) of merge_hash_kernel and merge_site_kernel in the context's last trgt_merge_exact_batch; both 0 unless
 * trgt_hip_timing_enable was on for that call.  cf. trgt_plot_kernel_ms */
int trgt_merge_kernel_ms(const trgt_hip_ctx* ctx, double out[2]);
#endif
