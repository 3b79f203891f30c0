/* trgt_hip_merge_sites.h -- the merge path in front of merge_exact: what merge_variants / merge_variant of `trgt merge`
 * (src/merge/vcf_processor.rs:237-299, 350-415, 452-532, 570-656) compute for one contig between reading the files' records and calling
 * merge_exact, as one call:
 *
 *   - the sites: which records of which files meet (the heap over positions, :242-285);
 *   - the padding base in front of the alleles of pre-1.0 files (add_padding_base, :350-388);
 *   - per site the concatenated entries: alleles, genotypes and the dense FORMAT rows of FormatData (process_record,
 *     process_missing_record, process_am_field, :452-494, :570-656), the genotypes already in the padded form of flatten_genotypes
 *     (:519-532);
 *   - the template record of each site (get_template_record, :436-439).
 *
 * Part of include/trgt_hip.h, which includes this file inside its extern "C" block behind trgt_hip_merge.h; not meant to be included
 * on its own.  Additions to ABI 11.  What the call leaves is a ready trgt_merge_in for trgt_merge_exact_batch.  Reading the VCFs, header
 * merging, the FORMAT strings themselves (ALLR / ALCI, MC, MS), skip_n / process_n and writing stay with the caller.
 *
 * Input.  One contig.  File f owns records [file_record_begin[f], file_record_begin[f + 1]) in file order; record r has position pos[r],
 * alleles [record_allele_begin[r], record_allele_begin[r + 1]) (REF first; allele a is the allele_len[a] bytes at allele_blob +
 * allele_off[a]) and, per numeric FORMAT field, n_samples(file of r) * width[r] values at values + begin[r], sample after sample, in BCF
 * layout: a sample with fewer values than the record's width is filled up with vector end (INT32_MIN + 1 in the integer fields,
 * 0x7F800002 in the float ones).  A RECORD-SAMPLE index counts the samples of all records in record order: record r, sample i is
 * sum over r' < r of n_samples(file of r') + i.
 *
 * Sites.  Positions never decrease inside a file (what an indexed fetch yields).  Then the heap of the reference, which holds one record
 * per file and pops every element at the smallest position, yields exactly the distinct keys (pos, k) in increasing order, k being a
 * record's rank among the records of its own file at that position; site (P, k) holds the k-th record at P of every file that has one.
 *
 * Vector end -- one reading that the reference's sources do not pin.  rust-htslib is not part of them.  The per-sample slices of
 * format(..).integer() / .float() and of genotypes().get(i) are taken to be CUT AT THE FIRST VECTOR-END VALUE; that is what gives the
 * reference's `sample_values.len() <= 1` rule (:595, :610, :650) a meaning.  It decides a result only in the padding test: a haploid
 * first sample with AL [0, vector end] in a width-2 record has the slice [0], minimum 0, and the record is NOT padded (with whole-width
 * slices the minimum would be vector end, and it would be).  Reproduced as read.
 *
 * Entries.  Site t has n_files entries, e = t * n_files + f, empty ones included (site_entry_begin[t] = t * n_files).  With
 * S = sum of n_samples and col(f, i) = sum over f' < f of n_samples[f'] + i, every row below has two values per sample at
 * (t * S + col) * 2:
 *   present record  the sample's slice [a, b] as it is; [a] becomes [a, vector end] (the <= 1 rule; for gt what flatten_genotypes
 *                   appends behind merge_exact, which passes vector end through).  am of a file with am_is_int: INT32_MIN becomes
 *                   0x7F800001, every other value the bits of (float)i / 255.0f, correctly rounded; the cut is at INT32_MIN + 1.
 *   absent record   gt [0, vector end] (UnphasedMissing); al, sd [INT32_MIN, INT32_MIN + 1]; ap, am [0x7F800001, 0x7F800002].
 * ap and am (float input) are moved as bit patterns: NaN payloads are data.  sample_src[t * S + col] is the record-sample index whose
 * ALLR / MC / MS strings belong there, -1 for "." (absent record).  Strings are not copied.  entry_gt_begin[e] = (t * S + col(f, 0)) * 2.
 *
 * Alleles.  The alleles of the present records in entry order: entry_allele_begin, allele_src (the input allele each one is),
 * allele_len, allele_off.  Padding applies to the present records of files with pre_v1: m is the minimum over the slice of the
 * record's first sample in al; if m != 0 every allele of the record, REF included, gets pad_base[r] in front (one byte, copied as
 * given).  If no file is pre_v1, allele_off points into the INPUT blob, nothing is copied and blob_written is 0.  Otherwise the
 * output blob receives all alleles, tightly packed in entry order, padded ones with their base in front; allele_off points into it
 * and blob_written is its length.  blob_cap must be at least sum of allele_len + the number of alleles of the records of pre_v1 files.
 *
 * Status.  site_stage_status[t] is 0 or TRGT_MERGE_SITE_RAGGED: a present record has a sample whose slice in gt or in a numeric field
 * is empty.  The reference would build ragged arrays that htslib refuses, or panic in the padding's unwrap.  It never fails the call;
 * the site's entries and alleles are still listed (a record whose first al slice is empty is not padded), its rows are unspecified.
 *
 * Sizing.  n_sites and record_site are always written.  If n_sites > cap_sites the call returns TRGT_ERR_NOMEM having written nothing
 * else; cap_sites = 0 with NULL site arrays is the sizing call.  Every other size follows from the input.  With n_sites <= cap_sites
 * the arrays are written for n_sites sites (the begin arrays: n_sites + 1 and n_sites * n_files + 1 elements).
 *
 * Errors.  Every check runs before the first launch and before any output is written; the message (trgt_hip_last_error) names the
 * first offender.  TRGT_ERR_INVALID: a NULL among the arrays that have elements; n_files < 0, cap_sites < 0, n_samples < 1; a begin
 * array that does not start at 0, decreases, or disagrees with n_samples * width; a width of 0; a position that decreases inside a
 * file or lies outside [0, 2^40); allele_off + allele_len > blob_len; a blob_cap too small although a file is pre_v1.
 * TRGT_ERR_UNSUPPORTED: a width above 2; more than 2^24 - 1 records of one file at one position; 2^31 - 16 or more records, alleles,
 * record-samples or files, or cap_sites * max(n_files, 2 * S) of 2^31 - 16 or more (32-bit indices in the kernels).
 * trgt_merge_sites_host has no context: it returns the same codes and leaves the message where trgt_hip_last_error(NULL) reads it. */
#ifndef TRGT_HIP_MERGE_SITES_H
#define TRGT_HIP_MERGE_SITES_H
#ifndef TRGT_HIP_H
#error "include trgt_hip.h, which includes this file"
#endif

#define TRGT_MERGE_SITE_RAGGED 4
#define TRGT_MERGE_MISSING_INTEGER (-2147483647 - 1)   /* INT32_MIN, bcf_int32_missing */
#define TRGT_MERGE_MISSING_FLOAT 0x7F800001u           /* bcf_float_missing */
#define TRGT_MERGE_VECTOR_END_FLOAT 0x7F800002u        /* bcf_float_vector_end */

typedef struct trgt_merge_field {      /* one numeric FORMAT field (or GT) of all records */
  const uint8_t* width;                /* [n_records] values per sample in that record: 1 or 2 */
  const uint64_t* begin;               /* [n_records + 1] into values; begin[r + 1] - begin[r] == n_samples(file of r) * width[r] */
  const void* values;                  /* int32 (GT, AL, SD, integer AM) or uint32 bit patterns (AP, float AM); BCF padding inside */
} trgt_merge_field;

typedef struct trgt_merge_sites_in {   /* one contig; every array host unless said otherwise */
  int32_t n_files;
  const int32_t* n_samples;            /* [n_files], >= 1 */
  const uint8_t* pre_v1;               /* [n_files] 1: version major < 1 (padding applies) */
  const uint8_t* am_is_int;            /* [n_files] 1: AM is the legacy integer field */
  const uint64_t* file_record_begin;   /* [n_files + 1] records of file f in file order */
  const int64_t* pos;                  /* [n_records] 0-based, never decreasing inside a file, 0 <= pos < 2^40 */
  const uint8_t* pad_base;             /* [n_records] read only for records of pre_v1 files; copied as given */
  const uint64_t* record_allele_begin; /* [n_records + 1] REF first */
  const uint64_t* allele_off;          /* [n_alleles] */
  const uint32_t* allele_len;          /* [n_alleles] */
  const uint8_t* allele_blob;          /* host or device (trgt_merge_sites_host: host) */
  uint64_t blob_len;
  trgt_merge_field gt, al, sd, ap, am;
} trgt_merge_sites_in;

typedef struct trgt_merge_sites_out {  /* S = sum of n_samples, n_alleles = record_allele_begin[n_records] */
  int64_t cap_sites;                   /* in: sites the site arrays hold */
  int64_t n_sites;                     /* out, always */
  int32_t* record_site;                /* [n_records] host, always written */
  int64_t* site_pos;                   /* [cap_sites] host */
  int32_t* site_template;              /* [cap_sites] host: the record of the first file that has one */
  int32_t* site_stage_status;          /* [cap_sites] host */
  int32_t* entry_record;               /* [cap_sites * n_files] host; -1: the file has no record there */
  uint64_t* site_entry_begin;          /* [cap_sites + 1] host           -- from here: the arrays of a trgt_merge_in */
  uint64_t* entry_allele_begin;        /* [cap_sites * n_files + 1] host */
  uint64_t* allele_off;                /* [n_alleles] host */
  uint32_t* allele_len;                /* [n_alleles] host */
  int32_t* allele_src;                 /* [n_alleles] host: the input allele */
  uint64_t* entry_gt_begin;            /* [cap_sites * n_files + 1] host */
  int32_t* gt;                         /* [cap_sites * S * 2] host */
  uint8_t* allele_blob;                /* [blob_cap] host or device (trgt_merge_sites_host: host); written only with a pre_v1 file */
  uint64_t blob_cap;
  uint64_t blob_written;               /* out */
  int32_t* al;                         /* [cap_sites * S * 2] host or device (trgt_merge_sites_host: host), as are the next four */
  int32_t* sd;
  uint32_t* ap;
  uint32_t* am;
  int32_t* sample_src;                 /* [cap_sites * S] */
} trgt_merge_sites_out;

/* merge_sites_key_kernel, the radix sort's three kernels, merge_sites_head_kernel, merge_sites_fill_kernel, merge_sites_allele_kernel
 * and merge_sites_copy_kernel (csrc/merge_sites.hip); synchronous on the context's stream */
int trgt_merge_sites_batch(trgt_hip_ctx* ctx, const trgt_merge_sites_in* in, trgt_merge_sites_out* out);
/* The host twin: the same results on one thread.  No context, no GPU, host pointers only */
int trgt_merge_sites_host(const trgt_merge_sites_in* in, trgt_merge_sites_out* out);
/* Of the context's last trgt_merge_sites_batch: sites, sites with a stage status, padded records, blob bytes written */
int trgt_merge_sites_stats(const trgt_hip_ctx* ctx, int64_t out[4]);
/* Device time (ms) of the context's last trgt_merge_sites_batch: grouping (keys, sort, heads), fill (rows, entries, allele lists and
 * offsets), blob copy; all 0 unless trgt_hip_timing_enable was on for that call */
int trgt_merge_sites_kernel_ms(const trgt_hip_ctx* ctx, double out[3]);
#endif
