"""Call time of deep Genotyper::Size loci: one blocking trgt_locus_batch call on one
context, reads resident in HBM, default max_depth (250), over 200 loci of 300 reads and over 200 loci of 750 reads, each with clean reads
(every read carries one of two exact alleles: majority support, no repair) and with noisy ones (3 % substitutions: the picks go through
the consensus repair).  Median of 20 calls after 5 warm-up calls, the spread of the 20, and the stats[4..8] split of the last call
(host waits for stage A, for stage B, for stage C, host glue, whole call, in ns).

SIZE_MAX_READS=<n>: the context's trgt_hip_set_size_max_reads setting (default: the library's default, 256 -- the host path).  A library
without the setter (the parent commit's) runs with no setting at all.  SIZE_DEEP_LOCI=<n>: loci per batch (default 200)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, locus  # noqa: E402

A, B = b"CAG" * 8 + b"CCG" * 3, b"CAG" * 8 + b"CCG" * 9


def batch(n_loci, n_reads, rate, seed):
    rng = np.random.default_rng(seed)
    dna = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    noisy = lambda rep: bytes(int(rng.choice(list(b"ACGT"))) if rng.random() < rate else c for c in rep) if rate else rep
    loci = []
    for _ in range(n_loci):
        lf, rf = dna(250), dna(250)
        loci.append(dict(left_flank=lf, right_flank=rf, motifs=[b"CAG", b"CCG"], genotyper="size", tr=A,
                         reads=[dna(int(rng.integers(250, 300))) + lf + noisy(A if i % 2 else B) + rf + dna(int(rng.integers(250, 300))) for i in range(n_reads)]))
    return locus.pack(loci)


def main():
    import torch
    n_loci = int(os.environ.get("SIZE_DEEP_LOCI", "200"))
    setting = os.environ.get("SIZE_MAX_READS")
    ctx = _lib.Context(0)
    if setting is not None:
        ctx.set_size_max_reads(int(setting))
    print("device: %s; size_max_reads: %s; %d loci per batch; default max_depth" % (torch.cuda.get_device_name(0), setting or "library default", n_loci), flush=True)
    params = locus.Params()
    for n_reads in (300, 750):
        for name, rate in (("clean", 0.0), ("noisy", 0.03)):
            b = batch(n_loci, n_reads, rate, seed=11 + n_reads)
            reads_dev = torch.from_numpy(b["read_blob"]).cuda()
            flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
            out = locus.BatchOutputs(b)
            times = []
            for _ in range(25):
                t0 = time.perf_counter()
                locus.run_batch(b, params, ctx=ctx, outputs=out, flank_dev=flank_dev, reads_dev=reads_dev)
                times.append((time.perf_counter() - t0) * 1e3)
            timed = times[5:]
            deep = ctx.size_deep_stats() if hasattr(ctx, "size_deep_stats") else None
            print("%4d reads %-5s: median %8.2f ms  (min %.2f, max %.2f of 20)  stats[4..8] = %s  repair loci %d  deep stats %s  checksum %d" % (
                n_reads, name, statistics.median(timed), min(timed), max(timed), " ".join(str(int(v)) for v in out.stats[4:9]), int(out.stats[18]), deep,
                int(out.allele_len.astype(np.int64).sum()) * 31 + int((out.classification.astype(np.int64) + 1).sum())), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
