"""Call time of haplotagged input: one blocking trgt_locus_batch call on one context, the cfg2 synthetic batch
(10 000 loci, 30 reads each) with its reads resident in HBM, run three ways:
  (a) no tags                                         -- the floor: genotype_flank has nothing to read;
  (b) hp_tag = read index in locus % 2 + 1, setting off -- every close-allele locus is genotyped again on the host path;
  (c) the same tags, trgt_hip_set_flank_device on       -- the tag split runs inside the device genotyper.
(b) and (c) run on two contexts that alternate in one process, call by call.  Median (min .. max) of 20 calls after 5 warm-up calls,
trgt_hip_flank_stats and the host time inside the call (stats[7], the host glue of the host path) of the last call.

Tagging EVERY read sends every locus with two close alleles down the route: this is the upper bound of the effect, not a model of a
real sample.  FLANK_TIMING_LOCI=<n>: loci per batch (default 10 000)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, locus, synth  # noqa: E402

CALLS, WARMUP = 20, 5


def line(name, times, out, ctx):
    print("%-34s median %7.2f ms  (min %.2f .. max %.2f of %d)  host glue %6.2f ms  repair loci %d  flank_stats %s  checksum %d" % (
        name, statistics.median(times), min(times), max(times), len(times), int(out.stats[7]) / 1e6, int(out.stats[18]), ctx.flank_stats(),
        int(out.allele_len.astype(np.int64).sum()) * 31 + int((out.classification.astype(np.int64) + 1).sum())), flush=True)


def main():
    import torch
    n_loci = int(os.environ.get("FLANK_TIMING_LOCI", "10000"))
    b = synth.generate(n_loci, first_locus=0, config=2)
    lrb = b["locus_read_begin"].astype(np.int64)
    nr = int(lrb[n_loci])
    tagged = dict(b)
    tagged.pop("_cin", None)
    idx = np.arange(nr, dtype=np.int64) - np.repeat(lrb[:-1], np.diff(lrb))
    tagged["hp_tag"] = (idx % 2 + 1).astype(np.int16)
    tagged["start_offset"] = np.zeros(nr, np.int32)
    tagged["end_offset"] = np.zeros(nr, np.int32)
    reads_dev = torch.from_numpy(b["read_blob"]).cuda()
    flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
    params = locus.Params()
    print("device: %s; %d loci, %d reads; reads resident in HBM; %d calls after %d warm-up calls" % (torch.cuda.get_device_name(0), n_loci, nr, CALLS, WARMUP), flush=True)
    print("every read is tagged: the upper bound of the effect, not a model of a real sample", flush=True)
    plain_ctx, off_ctx, on_ctx = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    on_ctx.set_flank_device(True)

    def call(ctx, batch, out):
        t0 = time.perf_counter()
        locus.run_batch(batch, params, ctx=ctx, outputs=out, flank_dev=flank_dev, reads_dev=reads_dev)
        return (time.perf_counter() - t0) * 1e3

    out_a = locus.BatchOutputs(b)
    ta = [call(plain_ctx, b, out_a) for _ in range(WARMUP + CALLS)][WARMUP:]
    line("(a) no tags", ta, out_a, plain_ctx)
    out_b, out_c = locus.BatchOutputs(tagged), locus.BatchOutputs(tagged)
    tb, tc = [], []
    for _ in range(WARMUP + CALLS):  # alternating, call by call
        tb.append(call(off_ctx, tagged, out_b))
        tc.append(call(on_ctx, tagged, out_c))
    line("(b) all tagged, setting off", tb[WARMUP:], out_b, off_ctx)
    line("(c) all tagged, setting on", tc[WARMUP:], out_c, on_ctx)
    same = all(np.array_equal(getattr(out_b, k), getattr(out_c, k)) for k in ("n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "gt_size", "flipped", "n_spans", "motif_counts"))
    print("(b) and (c) give the same records: %s" % same, flush=True)
    for c in (plain_ctx, off_ctx, on_ctx):
        c.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
