"""Call time of deep, un-tagged Genotyper::Size loci that carry mismatch offsets: one blocking trgt_locus_batch call
on one context, reads resident in HBM, default max_depth (250), over batches of loci of 300, 513 and 750 reads.  Every read carries one of
two exact alleles three bases apart; on half of the loci every other read carries a heterozygous pair of flank SNVs (-120, 85) and every
read a homozygous site (-200), on every locus a tenth of the reads one offset of their own.  Two contexts alternate call by call:
  on   trgt_hip_set_size_max_reads (the ceiling) and trgt_hip_set_snv_split_device: the SNV forms of the deep size kernels;
  off  trgt_hip_set_size_max_reads alone: the deep kernels genotype the locus, the host's flank step looks at every close-allele locus
       and genotypes the loci whose SNVs split the reads again on the host path.
Median (min .. max) of 20 calls after 5 warm-up calls, trgt_hip_snv_split_stats, trgt_hip_size_deep_stats and the host glue (stats[7]) of
the last call; the two contexts must give the same records.

TRGT_HIP_LIB=<path> loads another build (the parent commit's, where `on` is what such a context did before: the device genotypes, the
host looks again).  Run the libraries alternately, several processes each: the spread between processes is part of the result.
SNV_DEEP_LOCI=<n>: loci per batch (default 100).  SNV_DEEP_READS=<n>[,<n>...]: depths (default 300,513,750)."""
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
    for l in range(n_loci):
        lf, rf = dna(250), dna(250)
        het = l % 2 == 0
        reads, mm = [], []
        for i in range(n_reads):
            reads.append(dna(20) + lf + (A if i % 2 == 0 else B) + rf + dna(20))
            mm.append(sorted(([-200] if het else []) + ([-120, 85] if het and i % 2 else []) + ([int(rng.integers(90, 250))] if rng.random() < 0.1 else [])))
        loci.append(dict(left_flank=lf, right_flank=rf, motifs=[b"CAG"], genotyper="size", tr=A, ploidy=2, reads=reads, hp_tag=None,
                         start_offset=[-260] * n_reads, end_offset=[260] * n_reads, mismatch_offsets=mm))
    return locus.pack(loci)


def main():
    import torch
    from trgt_amd import _lib, locus
    n_loci = int(os.environ.get("SNV_DEEP_LOCI", "100"))
    depths = [int(v) for v in os.environ.get("SNV_DEEP_READS", "300,513,750").split(",")]
    on, off = _lib.Context(0), _lib.Context(0)
    on.set_size_max_reads(_lib.size_max_reads_limit()); on.set_snv_split_device(True)
    off.set_size_max_reads(_lib.size_max_reads_limit())
    print("device: %s; library: %s; %d loci per batch, half of them heterozygous at flank SNVs; reads resident in HBM; default max_depth; %d calls after %d warm-up calls" % (
        torch.cuda.get_device_name(0), os.environ.get("TRGT_HIP_LIB", "this tree's"), n_loci, CALLS, WARMUP), flush=True)
    params = locus.Params()
    ok = True
    for n_reads in depths:
        b = batch(locus, n_loci, n_reads, seed=29 + n_reads)
        reads_dev = torch.from_numpy(b["read_blob"]).cuda()
        flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
        outs = {"on": locus.BatchOutputs(b), "off": locus.BatchOutputs(b)}
        times = {"on": [], "off": []}
        for _ in range(WARMUP + CALLS):  # alternating, call by call
            for name, ctx in (("off", off), ("on", on)):
                t0 = time.perf_counter()
                locus.run_batch(b, params, ctx=ctx, outputs=outs[name], flank_dev=flank_dev, reads_dev=reads_dev)
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name, ctx in (("off", off), ("on", on)):
            t, out = times[name][WARMUP:], outs[name]
            print("%4d reads %-3s: median %8.2f ms  (min %.2f .. max %.2f of %d)  host glue %7.2f ms  snv_split_stats %s  size_deep_stats %s  checksum %d" % (
                n_reads, name, statistics.median(t), min(t), max(t), len(t), int(out.stats[7]) / 1e6, ctx.snv_split_stats(), ctx.size_deep_stats(),
                int(out.allele_len.astype(np.int64).sum()) * 31 + int((out.classification.astype(np.int64) + 1).sum())), flush=True)
        same = all(np.array_equal(getattr(outs["on"], k), getattr(outs["off"], k)) for k in FIELDS)
        print("%4d reads: on and off give the same records: %s" % (n_reads, same), flush=True)
        ok = ok and same
    on.close(); off.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
