"""Call time of un-tagged DEEP Genotyper::Cluster loci whose flank SNVs split their reads: one blocking
trgt_locus_batch call on ONE context set with cluster_max_reads = 2048, on the workload of tools/flank_cluster_deep_timing.py with
mismatch lists instead of tags -- 64 heterozygous cluster loci of 600 reads each (alleles CAG x 20 / CAG x 21 behind 250-base flanks,
0.5 % substitutions per read, so that most reads of a group but not all carry its sequence), max_depth = 10000 (every read is kept), the
reads resident in HBM.  No read carries a haplotype tag; every read has a mismatch at offset -200, the reads of the longer allele two more
at -120 and 85, so the SNV branch splits every locus.  trgt_hip_set_snv_cluster_deep_device alternates off / on on the same context, call
by call after warm-up calls in both settings; REPEATS calls each.  Off is the path of the commit before the setting existed: the deep chain
genotypes the loci and the host redoes them.  Reported: median (min .. max), trgt_hip_snv_cluster_deep_stats, the host time inside the
call (stats[7]), the loci the device chains completed (stats[22]) and the consensus alignments (stats[1]) of the last call, whether both
settings give the same records, and whether the two ranges overlap.  The lines are also written to the file named by the first argument
(default: profiles/snv_cluster_deep_timing.txt).

SNV_CLUSTER_DEEP_TIMING_LOCI=<n>: loci per batch (default 64).  SNV_CLUSTER_DEEP_TIMING_READS=<n>: reads per locus (default 600).
SNV_CLUSTER_DEEP_TIMING_REPEATS=<n>: calls per setting (default 4, at least 4).  SNV_CLUSTER_DEEP_TIMING_OFF_ONLY=1: only the setting-off
calls, without touching the setter -- the same batch on a library from before the setting, for the comparison with the parent commit."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trgt_amd import _lib, locus  # noqa: E402

WARMUP = 3
KEYS = ("n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "gt_size", "flipped", "n_spans", "motif_counts")


def dna(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tolist())


def make_locus(rng, n_reads):
    lf, rf = dna(rng, 250), dna(rng, 250)
    reads, hp, so, eo = [], [], [], []
    for i in range(n_reads):
        seg = bytearray(b"CAG" * (20 + i % 2))
        for p in np.flatnonzero(rng.random(len(seg)) < 0.005):
            seg[p] = ord("T")
        lc, rc = int(rng.integers(260, 400)), int(rng.integers(260, 400))
        reads.append(dna(rng, lc - 250) + lf + bytes(seg) + rf + dna(rng, rc - 250))
        hp.append(None)
        so.append(-lc); eo.append(rc)
    return dict(left_flank=lf, right_flank=rf, tr=b"CAG" * 20, motifs=[b"CAG"], ploidy=2, reads=reads, genotyper="cluster", hp_tag=hp,
                start_offset=so, end_offset=eo, mismatch_offsets=[[-200, -120, 85] if i % 2 else [-200] for i in range(n_reads)])


def main():
    import torch
    n_loci = int(os.environ.get("SNV_CLUSTER_DEEP_TIMING_LOCI", "64"))
    n_reads = int(os.environ.get("SNV_CLUSTER_DEEP_TIMING_READS", "600"))
    repeats = max(4, int(os.environ.get("SNV_CLUSTER_DEEP_TIMING_REPEATS", "4")))
    off_only = os.environ.get("SNV_CLUSTER_DEEP_TIMING_OFF_ONLY", "") == "1"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "snv_cluster_deep_timing.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(20251020)
    b = locus.pack([make_locus(rng, n_reads) for _ in range(n_loci)])
    reads_dev = torch.from_numpy(b["read_blob"]).cuda()
    flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
    params = locus.Params(max_depth=10000)
    say("python tools/snv_cluster_deep_timing.py%s -- device: %s" % (" (setting-off calls only)" if off_only else "", torch.cuda.get_device_name(0)))
    say("%d cluster loci of %d reads (CAG x 20 / CAG x 21, 0.5 %% substitutions), %d reads, no tags, %d mismatch offsets; max_depth 10000, cluster_max_reads 2048; reads resident in HBM" % (
        n_loci, n_reads, n_loci * n_reads, int(b["mismatch_off"][-1])))
    say("one context, blocking calls, the setting alternates call by call; %d calls per setting after %d warm-up calls each" % (repeats, WARMUP))
    ctx = _lib.Context(0)
    ctx.set_cluster_max_reads(2048)
    settings = (False,) if off_only else (False, True)
    outs = {False: locus.BatchOutputs(b), True: locus.BatchOutputs(b)}
    times, info = {False: [], True: []}, {}
    for i in range(WARMUP + repeats):
        for on in settings:
            if not off_only:
                ctx.set_snv_cluster_deep_device(on)
            t0 = time.perf_counter()
            locus.run_batch(b, params, ctx=ctx, outputs=outs[on], flank_dev=flank_dev, reads_dev=reads_dev)  # (blocking: returns with the results on the host)
            ms = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                times[on].append(ms)
            info[on] = (ctx.snv_cluster_deep_stats() if not off_only else None, int(outs[on].stats[7]) / 1e6, int(outs[on].stats[22]), int(outs[on].stats[1]))
    for on in settings:
        t = times[on]
        say("setting %-3s  median %8.2f ms  (min %.2f .. max %.2f of %d)  host glue %7.2f ms  snv_cluster_deep_stats %s  stats[22] %d  consensus alignments %d" % (
            "on" if on else "off", statistics.median(t), min(t), max(t), len(t), info[on][1], info[on][0], info[on][2], info[on][3]))
    same = True
    if not off_only:
        same = all(np.array_equal(getattr(outs[False], k), getattr(outs[True], k)) for k in KEYS)
        say("both settings give the same records: %s" % same)
        apart = max(times[True]) < min(times[False]) or max(times[False]) < min(times[True])
        say("the ranges of the two settings %s" % ("do not overlap" if apart else "overlap: no difference is claimed"))
    ctx.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
