"""Call time of un-tagged Genotyper::Cluster loci with mismatch offsets: one blocking trgt_locus_batch call on one
context, the cfg5 synthetic batch (compound motif sets, cluster genotyper; 2 000 loci by default, 30 reads each) with its reads resident
in HBM, run three ways:
  (a) no read metadata                                       -- the floor: genotype_flank has nothing to read;
  (b) mismatch offsets, setting off                          -- the host's flank step looks at every cluster locus with two close alleles,
                                                                and the loci whose SNVs split the reads are genotyped again on the host path;
  (c) the same offsets, trgt_hip_set_snv_cluster_device on   -- the SNV branch runs behind the one-wave cluster chain.
The offsets are those of tools/snv_split_timing.py (with_offsets): on SNV_CLUSTER_TIMING_SHARE of the loci (default 0.5) every other read
carries a heterozygous pair and every read a homozygous site; on every locus a tenth of the reads carry one offset of their own.
(b) and (c) run on two contexts that alternate in one process, call by call.  Median (min .. max) of REPEATS calls after WARMUP warm-up
calls, trgt_hip_snv_cluster_stats, the host time inside the call (stats[7]) of the last call, whether (b) and (c) give the same records,
the ratio of the medians and whether the two ranges overlap.  The lines go to standard output and to the file named by the first
argument (default: profiles/snv_cluster_timing.txt).
SNV_CLUSTER_TIMING_LOCI=<n>: loci per batch.  SNV_CLUSTER_TIMING_REPEATS=<n>: calls per run (default 9, at least 9)."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from snv_split_timing import KEYS, with_offsets  # noqa: E402
from trgt_amd import _lib, locus, synth  # noqa: E402

WARMUP = 3


def main():
    import torch
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "snv_cluster_timing.txt")
    n_loci = int(os.environ.get("SNV_CLUSTER_TIMING_LOCI", "2000"))
    repeats = max(9, int(os.environ.get("SNV_CLUSTER_TIMING_REPEATS", "9")))
    share = float(os.environ.get("SNV_CLUSTER_TIMING_SHARE", "0.5"))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    b = synth.generate(n_loci, first_locus=0, config=5)
    m, n_snv = with_offsets(b, share)
    reads_dev = torch.from_numpy(b["read_blob"]).cuda()
    flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
    params = locus.Params()
    say("python tools/snv_cluster_timing.py -- device: %s" % torch.cuda.get_device_name(0))
    say("%d cluster loci (cfg5), %d reads; %d loci with a heterozygous SNV pair (share %.2f); reads resident in HBM; blocking calls, %d calls after %d warm-up calls" % (
        n_loci, int(b["n_reads"]), n_snv, share, repeats, WARMUP))
    plain_ctx, off_ctx, on_ctx = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    on_ctx.set_snv_cluster_device(True)

    def call(ctx, batch, out):
        t0 = time.perf_counter()
        locus.run_batch(batch, params, ctx=ctx, outputs=out, flank_dev=flank_dev, reads_dev=reads_dev)
        return (time.perf_counter() - t0) * 1e3

    def line(name, times, out, ctx):
        say("%-36s median %7.2f ms  (min %.2f .. max %.2f of %d)  host glue %6.2f ms  snv_cluster_stats %s  checksum %d" % (
            name, statistics.median(times), min(times), max(times), len(times), int(out.stats[7]) / 1e6, ctx.snv_cluster_stats(),
            int(out.allele_len.astype(np.int64).sum()) * 31 + int((out.classification.astype(np.int64) + 1).sum())))

    out_a = locus.BatchOutputs(b)
    ta = [call(plain_ctx, b, out_a) for _ in range(WARMUP + repeats)][WARMUP:]
    line("(a) no read metadata", ta, out_a, plain_ctx)
    out_b, out_c = locus.BatchOutputs(m), locus.BatchOutputs(m)
    tb, tc = [], []
    for _ in range(WARMUP + repeats):  # alternating, call by call
        tb.append(call(off_ctx, m, out_b))
        tc.append(call(on_ctx, m, out_c))
    tb, tc = tb[WARMUP:], tc[WARMUP:]
    line("(b) mismatch offsets, setting off", tb, out_b, off_ctx)
    line("(c) mismatch offsets, setting on", tc, out_c, on_ctx)
    same = all(np.array_equal(getattr(out_b, k), getattr(out_c, k)) for k in KEYS)
    say("(b) and (c) give the same records: %s" % same)
    say("median of (c) / median of (b): %.3f" % (statistics.median(tc) / statistics.median(tb)))
    if max(tc) < min(tb):
        say("the ranges of (b) and (c) do not overlap, (c) is below")
    else:
        say("the ranges of (b) and (c) overlap or (c) is not below: no gain is claimed")
    for c in (plain_ctx, off_ctx, on_ctx):
        c.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
