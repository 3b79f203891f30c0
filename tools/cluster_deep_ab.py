"""A/B of the deep cluster chain (profiles/cluster_deep_ab.txt): one blocking trgt_locus_batch call over 64 heterozygous
Genotyper::Cluster loci of 600 reads each, on one context with trgt_hip_set_cluster_max_reads at 256 (every locus on host threads between GPU
alignment batches) and at the compiled ceiling (the deep chain).  Median of 5 calls after 2 warm-up calls.  AB_QUICK=1: the deep setting only,
one timed call (for a run under rocprofv3 --kernel-trace --stats)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, locus  # noqa: E402


def batch(n_loci=64, n_reads=600, seed=7):
    rng = np.random.default_rng(seed)
    dna = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    noisy = lambda rep: bytes(int(rng.choice(list(b"ACGT"))) if rng.random() < 0.03 else c for c in rep)
    loci = []
    for _ in range(n_loci):
        lf, rf = dna(250), dna(250)
        loci.append(dict(left_flank=lf, right_flank=rf, motifs=[b"CAG", b"CCG"], genotyper="cluster", tr=b"CAG" * 8,
                         reads=[dna(int(rng.integers(250, 300))) + lf + noisy(b"CAG" * 8 + b"CCG" * (3 if i % 2 else 9)) + rf + dna(int(rng.integers(250, 300))) for i in range(n_reads)]))
    return locus.pack(loci)


def main():
    quick = os.environ.get("AB_QUICK", "0") not in ("", "0")
    b = batch()
    params = locus.Params(max_depth=10000)
    out = locus.BatchOutputs(b)
    results = {}
    for setting in ([_lib.cluster_max_reads_limit()] if quick else [256, _lib.cluster_max_reads_limit()]):
        ctx = _lib.Context(0)
        ctx.set_cluster_max_reads(setting)
        times = []
        for k in range(2 if quick else 7):
            t0 = time.perf_counter()
            locus.run_batch(b, params, ctx=ctx, outputs=out)
            times.append((time.perf_counter() - t0) * 1e3)
        timed = times[1:] if quick else times[2:]
        results[setting] = (out.n_alleles.copy(), out.allele_len.copy(), out.classification.copy(), out.read_rank.copy())
        print("cluster_max_reads %4d: median %.1f ms  (calls: %s)  stats[22] = %d, stats[23] = %d, edit distances %d" % (
            setting, statistics.median(timed), " ".join("%.1f" % t for t in times), int(out.stats[22]), int(out.stats[23]), int(out.stats[15])), flush=True)
        ctx.close()
    if len(results) == 2:
        a, c = results.values()
        print("results identical: %s" % all(np.array_equal(x, y) for x, y in zip(a, c)))


if __name__ == "__main__":
    main()
