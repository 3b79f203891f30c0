"""Call time of deep, haplotagged Genotyper::Size loci: one blocking trgt_locus_batch call on one context with
trgt_hip_set_flank_device and trgt_hip_set_size_max_reads (the ceiling) both set, reads resident in HBM, default max_depth (250), over 200
loci of 300 reads and over 200 loci of 750 reads.  Every read carries one of two exact alleles three bases apart and is tagged by allele:
every locus goes down the tag route of genotype_flank -- the upper bound of the effect, not a model of a real sample.  Median (min .. max)
of 20 calls after 5 warm-up calls, trgt_hip_flank_stats, trgt_hip_size_deep_stats and the host glue (stats[7]) of the last call.

The comparison is between libraries, one process each: TRGT_HIP_LIB=<path> loads another build (the parent commit's, where the deep loci
are genotyped on the device and then again on the host path).  Run the two sides alternately, several times each.
  flank_deep_timing.py --dump FILE      also writes the records of both batches to FILE (.npz)
  flank_deep_timing.py --compare A B    compares two such files; exit status 1 when they differ
FLANK_DEEP_LOCI=<n>: loci per batch (default 200)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, WARMUP = 20, 5
A, B = b"CAG" * 20, b"CAG" * 21
FIELDS = ("n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "gt_size", "flipped", "n_spans", "motif_counts")


def batch(locus, n_loci, n_reads, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    dna = lambda n: acgt[rng.integers(0, 4, n)].tobytes()
    loci = []
    for _ in range(n_loci):
        lf, rf = dna(250), dna(250)
        reads, so, eo = [], [], []
        for i in range(n_reads):
            lc, rc = int(rng.integers(260, 300)), int(rng.integers(260, 300))
            reads.append(dna(lc - 250) + lf + (A if i % 2 == 0 else B) + rf + dna(rc - 250))
            so.append(-lc); eo.append(rc)
        loci.append(dict(left_flank=lf, right_flank=rf, motifs=[b"CAG"], genotyper="size", tr=A, ploidy=2, reads=reads,
                         hp_tag=[i % 2 + 1 for i in range(n_reads)], start_offset=so, end_offset=eo, mismatch_offsets=[[] for _ in reads]))
    return locus.pack(loci)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    same = sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)
    print("%s and %s hold the same records: %s (%d arrays)" % (pa, pb, same, len(a.files)))
    return 0 if same else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    dump = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--dump" else None
    import torch
    from trgt_amd import _lib, locus
    n_loci = int(os.environ.get("FLANK_DEEP_LOCI", "200"))
    ctx = _lib.Context(0)
    ctx.set_flank_device(True)
    ctx.set_size_max_reads(_lib.size_max_reads_limit())
    print("device: %s; library: %s; both settings on; %d loci per batch; reads resident in HBM; default max_depth; %d calls after %d warm-up calls" % (
        torch.cuda.get_device_name(0), os.environ.get("TRGT_HIP_LIB", "this tree's"), n_loci, CALLS, WARMUP), flush=True)
    params = locus.Params()
    records = {}
    for n_reads in (300, 750):
        b = batch(locus, n_loci, n_reads, seed=23 + n_reads)
        reads_dev = torch.from_numpy(b["read_blob"]).cuda()
        flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
        out = locus.BatchOutputs(b)
        times = []
        for _ in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            locus.run_batch(b, params, ctx=ctx, outputs=out, flank_dev=flank_dev, reads_dev=reads_dev)
            times.append((time.perf_counter() - t0) * 1e3)
        timed = times[WARMUP:]
        print("%4d reads: median %8.2f ms  (min %.2f .. max %.2f of %d)  host glue %7.2f ms  flank_stats %s  size_deep_stats %s  checksum %d" % (
            n_reads, statistics.median(timed), min(timed), max(timed), len(timed), int(out.stats[7]) / 1e6, ctx.flank_stats(), ctx.size_deep_stats(),
            int(out.allele_len.astype(np.int64).sum()) * 31 + int((out.classification.astype(np.int64) + 1).sum())), flush=True)
        for k in FIELDS:
            records["%d_%s" % (n_reads, k)] = np.array(getattr(out, k))
    ctx.close()
    if dump:
        np.savez(dump, **records)
    return 0


if __name__ == "__main__":
    sys.exit(main())
