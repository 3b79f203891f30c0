"""Call time of haplotagged Genotyper::Cluster loci: one blocking trgt_locus_batch call on ONE context, the cfg5
synthetic batch (compound motif sets, cluster genotyper; 2 000 loci by default, 30 reads each) with its reads resident in HBM.  The reads
carry the generator's haplotype as HP tag, except every seventh read of a locus, which stays untagged (86 % tagged: the tags split every
locus, and what decides the route is whether the cluster genotyper's two alleles are within 10 bases -- the generator's allele
differences, not this tool, set that share).  trgt_hip_set_flank_cluster_device alternates off / on on the same context, call by call
after warm-up calls in both settings; REPEATS calls each.  Reported: median (min .. max), trgt_hip_flank_cluster_stats, the host time
inside the call (stats[7]) and the loci on the host path of the last call, and whether both settings give the same records.

FLANK_CLUSTER_TIMING_LOCI=<n>: loci per batch.  FLANK_CLUSTER_TIMING_REPEATS=<n>: calls per setting (default 9, at least 5)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, locus, synth  # noqa: E402

WARMUP = 3
KEYS = ("n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "gt_size", "flipped", "n_spans", "motif_counts")


def main():
    import torch
    n_loci = int(os.environ.get("FLANK_CLUSTER_TIMING_LOCI", "2000"))
    repeats = max(5, int(os.environ.get("FLANK_CLUSTER_TIMING_REPEATS", "9")))
    b = synth.generate(n_loci, first_locus=0, config=5)
    lrb = b["locus_read_begin"].astype(np.int64)
    nr = int(lrb[n_loci])
    idx = np.arange(nr, dtype=np.int64) - np.repeat(lrb[:-1], np.diff(lrb))
    tagged = {k: v for k, v in b.items() if k != "_cin"}
    tagged["hp_tag"] = np.where(idx % 7 == 6, -1, b["read_hap"][:nr].astype(np.int64) + 1).astype(np.int16)
    tagged["start_offset"] = np.zeros(nr, np.int32)
    tagged["end_offset"] = np.zeros(nr, np.int32)
    reads_dev = torch.from_numpy(b["read_blob"]).cuda()
    flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
    params = locus.Params()
    true_len = b["true_allele_len"].astype(np.int64).reshape(-1, 2)
    close = int((np.abs(true_len[:, 0] - true_len[:, 1]) <= 10).sum())
    print("device: %s; %d cluster loci (cfg5), %d reads, %.0f %% tagged; true alleles within 10 bases: %d loci; reads resident in HBM" % (
        torch.cuda.get_device_name(0), n_loci, nr, 100.0 * float((tagged["hp_tag"] > 0).mean()), close), flush=True)
    print("one context, blocking calls, the setting alternates call by call; %d calls per setting after %d warm-up calls each" % (repeats, WARMUP), flush=True)
    ctx = _lib.Context(0)
    outs = {False: locus.BatchOutputs(tagged), True: locus.BatchOutputs(tagged)}
    times, info = {False: [], True: []}, {}
    for i in range(WARMUP + repeats):
        for on in (False, True):
            ctx.set_flank_cluster_device(on)
            t0 = time.perf_counter()
            locus.run_batch(tagged, params, ctx=ctx, outputs=outs[on], flank_dev=flank_dev, reads_dev=reads_dev)
            ms = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[on].append(ms)
            info[on] = (ctx.flank_cluster_stats(), int(outs[on].stats[7]) / 1e6, int(outs[on].stats[22]), int(outs[on].stats[1]))
    for on in (False, True):
        t = times[on]
        print("setting %-3s  median %7.2f ms  (min %.2f .. max %.2f of %d)  host glue %6.2f ms  flank_cluster_stats %s  stats[22] %d  consensus alignments %d" % (
            "on" if on else "off", statistics.median(t), min(t), max(t), len(t), info[on][1], info[on][0], info[on][2], info[on][3]), flush=True)
    same = all(np.array_equal(getattr(outs[False], k), getattr(outs[True], k)) for k in KEYS)
    print("both settings give the same records: %s" % same, flush=True)
    apart = max(times[True]) < min(times[False]) or max(times[False]) < min(times[True])
    print("the ranges of the two settings %s" % ("do not overlap" if apart else "overlap: no difference is claimed"), flush=True)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
