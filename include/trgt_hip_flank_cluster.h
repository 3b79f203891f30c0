/* trgt_hip_flank_cluster.h -- the two entry points of the haplotype-tag branch of genotype_flank behind the device cluster chain
 * (genotype_flank.rs:9-76, 147-170; tr.rs:64-75).  Part of include/trgt_hip.h, which includes this file inside its extern "C" block and
 * documents both functions (what runs on the device, what stays on the host, the three counts); not meant to be included on its own.
 * Additions to ABI 11. */
#ifndef TRGT_HIP_FLANK_CLUSTER_H
#define TRGT_HIP_FLANK_CLUSTER_H
#ifndef TRGT_HIP_H
#error "include trgt_hip.h, which includes this file"
#endif
int trgt_hip_set_flank_cluster_device(trgt_hip_ctx* ctx, int on);
int trgt_hip_flank_cluster_stats(const trgt_hip_ctx* ctx, int64_t out[3]);
#endif
