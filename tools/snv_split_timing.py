"""Call time of un-tagged input with mismatch offsets: one blocking trgt_locus_batch call on one context, the cfg2
synthetic batch (1 000 and 10 000 loci, 30 reads each) with its reads resident in HBM, run three ways:
  (a) no read metadata                                     -- the floor: genotype_flank has nothing to read;
  (b) mismatch offsets, setting off                        -- the host's flank step looks at every close-allele locus and the loci whose
                                                              SNVs split the reads are genotyped again on the host path;
  (c) the same offsets, trgt_hip_set_snv_split_device on   -- the SNV branch runs inside the device genotyper.
The offsets are made the way tests/test_flank_gpu._phased_locus makes them: on SNV_TIMING_SHARE of the loci (default 0.5) every other read
carries a heterozygous pair (-120, 85) and every read a homozygous site (-200); on every locus a tenth of the reads carry one offset of
their own (a sequencing error).  start_offset / end_offset are -250 / 250.
(b) and (c) run on two contexts that alternate in one process, call by call.  Median (min .. max) of 20 calls after 5 warm-up calls,
trgt_hip_snv_split_stats, trgt_hip_flank_stats and the host time inside the call (stats[7], the host glue of the host path) of the last
call.  SNV_TIMING_LOCI=<n>[,<n>...]: loci per batch (default 1000,10000)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, locus, synth  # noqa: E402

CALLS, WARMUP = 20, 5
KEYS = ("n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "gt_size", "flipped", "n_spans", "motif_counts")


def line(name, times, out, ctx):
    print("%-36s median %7.2f ms  (min %.2f .. max %.2f of %d)  host glue %6.2f ms  snv_split_stats %s  flank_stats %s  checksum %d" % (
        name, statistics.median(times), min(times), max(times), len(times), int(out.stats[7]) / 1e6, ctx.snv_split_stats(), ctx.flank_stats(),
        int(out.allele_len.astype(np.int64).sum()) * 31 + int((out.classification.astype(np.int64) + 1).sum())), flush=True)


def with_offsets(b, share, seed=7):
    rng = np.random.default_rng(seed)
    n_loci = int(b["n_loci"])
    lrb = b["locus_read_begin"].astype(np.int64)
    nr = int(lrb[n_loci])
    m = dict(b)
    m.pop("_cin", None)
    snv_locus = rng.random(n_loci) < share
    idx = np.arange(nr, dtype=np.int64) - np.repeat(lrb[:-1], np.diff(lrb))
    on = np.repeat(snv_locus, np.diff(lrb))
    err = rng.random(nr) < 0.1
    err_at = rng.integers(90, 250, nr)
    mm, off = [], [0]
    for r in range(nr):
        lst = ([-200] if on[r] else []) + ([-120, 85] if on[r] and idx[r] % 2 else []) + ([int(err_at[r])] if err[r] else [])
        mm += sorted(lst)
        off.append(len(mm))
    m["start_offset"] = np.full(nr, -250, np.int32)
    m["end_offset"] = np.full(nr, 250, np.int32)
    m["mismatch_offsets"] = np.array(mm + [0], np.int32)
    m["mismatch_off"] = np.array(off, np.uint64)
    return m, int(snv_locus.sum())


def run(n_loci, share, torch):
    b = synth.generate(n_loci, first_locus=0, config=2)
    m, n_snv = with_offsets(b, share)
    reads_dev = torch.from_numpy(b["read_blob"]).cuda()
    flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
    params = locus.Params()
    print("---- %d loci, %d reads; %d loci with a heterozygous SNV pair (share %.2f); reads resident in HBM; %d calls after %d warm-up calls" % (
        n_loci, int(b["n_reads"]), n_snv, share, CALLS, WARMUP), flush=True)
    plain_ctx, off_ctx, on_ctx = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    on_ctx.set_snv_split_device(True)

    def call(ctx, batch, out):
        t0 = time.perf_counter()
        locus.run_batch(batch, params, ctx=ctx, outputs=out, flank_dev=flank_dev, reads_dev=reads_dev)
        return (time.perf_counter() - t0) * 1e3

    out_a = locus.BatchOutputs(b)
    ta = [call(plain_ctx, b, out_a) for _ in range(WARMUP + CALLS)][WARMUP:]
    line("(a) no read metadata", ta, out_a, plain_ctx)
    out_b, out_c = locus.BatchOutputs(m), locus.BatchOutputs(m)
    tb, tc = [], []
    for _ in range(WARMUP + CALLS):  # alternating, call by call
        tb.append(call(off_ctx, m, out_b))
        tc.append(call(on_ctx, m, out_c))
    line("(b) mismatch offsets, setting off", tb[WARMUP:], out_b, off_ctx)
    line("(c) mismatch offsets, setting on", tc[WARMUP:], out_c, on_ctx)
    same = all(np.array_equal(getattr(out_b, k), getattr(out_c, k)) for k in KEYS)
    print("(b) and (c) give the same records: %s" % same, flush=True)
    for c in (plain_ctx, off_ctx, on_ctx):
        c.close()
    return same


def main():
    import torch
    share = float(os.environ.get("SNV_TIMING_SHARE", "0.5"))
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    ok = True
    for n in [int(v) for v in os.environ.get("SNV_TIMING_LOCI", "1000,10000").split(",")]:
        ok = run(n, share, torch) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
