/* trgt_hip_flank_cluster.h -- the entry points of genotype_flank behind the device cluster chain: the two of the haplotype-tag branch
 * (genotype_flank.rs:9-76, 147-170; tr.rs:64-75), which include/trgt_hip.h documents (what runs on the device, what stays on the host,
 * the three counts), the two of the SNV branch, the two of the tag branch behind the deep chain and the two of the SNV branch behind it, documented below.  Part of include/trgt_hip.h, which includes this file inside its
 * extern "C" block; not meant to be included on its own.  Additions to ABI 11. */
#ifndef TRGT_HIP_FLANK_CLUSTER_H
#define TRGT_HIP_FLANK_CLUSTER_H
#ifndef TRGT_HIP_H
#error "include trgt_hip.h, which includes this file"
#endif
int trgt_hip_set_flank_cluster_device(trgt_hip_ctx* ctx, int on);
int trgt_hip_flank_cluster_stats(const trgt_hip_ctx* ctx, int64_t out[3]);
/* The other branch of the same step for Genotyper::Cluster loci: the split by heterozygous SNVs of the flanks (get_trs_with_clustering
 * with its analysis region, SNV calls, profiles, candidate genotypes and log-likelihoods, genotype_flank.rs:78-138, 171-290; applied by
 * analyze at tr.rs:64-75 whichever genotyper produced the alleles).  A setting of its own, independent of the three others.  By default
 * the host runs this step for every device-genotyped cluster locus with two alleles at most 10 bases apart, and redoes the loci whose
 * SNVs split the reads from the start.  On a context set with on != 0, calls whose batch carries mismatch_offsets and mismatch_off run
 * it behind the one-wave cluster chain (the SNV forms of locus_cluster_flank.hpp) for the cluster loci of ploidy 2 and at most 256
 * candidate reads, in the reference's order, tags first: tags that split the reads own the locus (the device's tag branch with
 * trgt_hip_set_flank_cluster_device also on, else the host as before), the SNVs are tried only without them.  The search is the one of
 * trgt_hip_set_snv_split_device, stated once: everything but exp and log is restated bit for bit, and it is decided on the device only
 * when its winner is ahead of every other candidate by more than 2^-30 * (1 + |log-likelihood|).  The groups of this branch overlap: a
 * read that agrees equally with both haplotypes is a member of both; consensus, intervals and the third consensus round follow the
 * membership, num_spanning and the classification the assignment.
 * What stays on the host, with the same results: deep cluster loci (257 to 2048 reads on a context set with
 * trgt_hip_set_cluster_max_reads), in both branches unless the context is also set with trgt_hip_set_flank_cluster_deep_device (below),
 * which runs the tag branch for them, or with trgt_hip_set_snv_cluster_deep_device (below), which runs the SNV branch; contexts created under TRGT_HOST_CLUSTER or TRGT_HOST_GENOTYPER; searches not
 * decided beyond the margin; loci beyond one of the three limits -- more than 64 called SNVs, more than 16 distinct fully observed
 * profiles, more than 8 in-region mismatch offsets per candidate read slot of the kernel form (512 / 2048 occurrences per locus for
 * the 64-read / 256-read forms); a locus on this route that finds no room in the chain's arenas, whose repaired group overflows its
 * slot, or that has an allele beyond allele_cap; and the tag branch where trgt_hip_set_flank_cluster_device is off.
 * trgt_hip_snv_cluster_stats: of the context's last trgt_locus_batch -- out[0] cluster loci whose genotype the device replaced through
 * the SNV branch, out[1] those among them with a repaired group, out[2] loci on the route handed back for room or limits, out[3] loci
 * handed back because the search was not decided beyond the margin (not in out[2]); all zero with the setting off, a batch without
 * mismatch offsets or a call without a device cluster chain.  A locus this branch settles or hands back is in no other count:
 * trgt_hip_flank_cluster_stats counts the tag branch only, trgt_hip_snv_split_stats and trgt_hip_flank_stats never a cluster locus. */
int trgt_hip_set_snv_cluster_device(trgt_hip_ctx* ctx, int on);
int trgt_hip_snv_cluster_stats(const trgt_hip_ctx* ctx, int64_t out[4]);
/* The haplotype-tag branch (genotype_flank.rs:9-76, 147-170; tr.rs:64-75) for DEEP cluster loci: Genotyper::Cluster loci of 257 to 2048
 * candidate reads, which the seven-kernel deep chain genotypes on a context set with trgt_hip_set_cluster_max_reads.  A setting of its own,
 * off by default and independent of the four others: it is not what trgt_hip_set_flank_cluster_device and
 * trgt_hip_set_cluster_max_reads give together, and contexts with those two behave as they always did.  By default the host, where the
 * tags split the reads of such a locus, redoes it from the start. */
int trgt_hip_set_flank_cluster_deep_device(trgt_hip_ctx* ctx, int on);
/* On a context set with on != 0 that also has a deep cluster chain, calls whose batch carries hp_tag run the tag branch behind that chain
 * (locus_cluster_flank_deep.hpp, one workgroup per locus) for the loci of the deep list with ploidy 2 and two alleles at most 10 bases
 * apart: assignment by tag with the rule of the deep size route, acceptance (both groups occur, 70 % of the kept reads tagged),
 * simple_consensus of either group -- equal sequences found in the read blob through (length, hash) pairs and confirmed byte by byte --,
 * a third consensus round of the deep list for a group without a majority sequence, smaller allele first, reference allele first.
 * What stays on the host, with the same results: the SNV-clustering branch (get_trs_with_clustering) for deep cluster loci, tried for
 * the loci whose tags do not split the reads exactly as before unless the context is also set with
 * trgt_hip_set_snv_cluster_deep_device (below); loci beyond the context's cluster_max_reads setting or the ceiling of
 * 2048 reads; deep loci that found no room in the call's pair budget; contexts created under TRGT_HOST_CLUSTER or TRGT_HOST_GENOTYPER;
 * and the hand-backs -- a locus on this route that finds no room in the deep chain's arenas, whose repaired group overflows its slot, or
 * that has an allele beyond allele_cap.
 * trgt_hip_flank_cluster_deep_stats: of the context's last trgt_locus_batch -- out[0] deep cluster loci whose genotype the device
 * replaced by the tag split, out[1] those among them with at least one repaired group, out[2] deep cluster loci on the route that the
 * device handed back to the host path; all zero with the setting off, a batch without hp_tag or a call without a deep cluster list.
 * These loci are in no other count: not in trgt_hip_flank_cluster_stats, not in trgt_hip_flank_stats, not in stats[23]. */
int trgt_hip_flank_cluster_deep_stats(const trgt_hip_ctx* ctx, int64_t out[3]);
/* The SNV branch (get_trs_with_clustering, genotype_flank.rs:78-138, 171-290; applied by analyze at tr.rs:64-75) for DEEP cluster loci:
 * Genotyper::Cluster loci of 257 to 2048 candidate reads on a context set with trgt_hip_set_cluster_max_reads.  A setting of its own, off
 * by default and independent of the five others.  It combines with trgt_hip_set_cluster_max_reads, which it follows (without a deep
 * cluster chain it does nothing), and with trgt_hip_set_flank_cluster_deep_device, which says whose the tag branch of these loci is: the
 * device's with both settings on, else the host's as before.  By default the host, where the SNVs split the reads of such a locus, redoes
 * it from the start. */
int trgt_hip_set_snv_cluster_deep_device(trgt_hip_ctx* ctx, int on);
/* On a context set with on != 0 that also has a deep cluster chain, calls whose batch carries mismatch_offsets and mismatch_off run the
 * branch behind that chain (the SNV forms of locus_cluster_flank_deep.hpp, one workgroup per locus) for the loci of the deep list with
 * ploidy 2 and two alleles at most 10 bases apart, in the reference's order, tags first: tags that split the reads own the locus, the
 * SNVs are tried only without them.  The search is the one of the deep size route (trgt_hip_set_snv_split_device with
 * trgt_hip_set_size_max_reads), stated once: analysis region, SNV calls, profiles, candidate genotypes, log-likelihoods, decided on the
 * device only when the winner is ahead of every other candidate by more than 2^-30 * (1 + |log-likelihood|).  Its groups overlap: a read
 * that agrees equally with both haplotypes is a member of both; simple_consensus, intervals and the third consensus round of the deep
 * list follow the membership, num_spanning and the classification the assignment; smaller allele first, reference allele first.
 * What stays on the host, with the same results: searches not decided beyond the margin; loci beyond one of the three limits -- more
 * than 64 called SNVs, more than 16 distinct fully observed profiles, more than 16384 in-region mismatch offsets per locus; the tag
 * branch where trgt_hip_set_flank_cluster_deep_device is off; loci beyond the context's cluster_max_reads setting or the ceiling of 2048
 * reads; deep loci that found no room in the call's pair budget; contexts created under TRGT_HOST_CLUSTER or TRGT_HOST_GENOTYPER; and
 * the hand-backs -- a locus on this route that finds no room in the deep chain's arenas, whose repaired group overflows its slot, or
 * that has an allele beyond allele_cap.
 * trgt_hip_snv_cluster_deep_stats: of the context's last trgt_locus_batch -- out[0] deep cluster loci whose genotype the device replaced
 * through the SNV branch, out[1] those among them with a repaired group, out[2] loci on the route handed back for room or limits, out[3]
 * loci handed back because the search was not decided beyond the margin (not in out[2]); all zero with the setting off, a batch without
 * mismatch offsets or a call without a deep cluster list.  These loci are in no other count: not in trgt_hip_flank_cluster_deep_stats
 * (which keeps counting the tag branch only), trgt_hip_snv_cluster_stats, trgt_hip_flank_cluster_stats, trgt_hip_flank_stats or
 * stats[23]. */
int trgt_hip_snv_cluster_deep_stats(const trgt_hip_ctx* ctx, int64_t out[4]);
#endif
