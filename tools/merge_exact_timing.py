"""Call time of trgt_merge_exact_batch on two synthetic cohorts, with its host twin beside it for orientation.

  STR catalog       2 000 sites x 1 000 single-sample entries x (REF + 2 ALTs); the ALTs of a site are drawn, skewed, from about 20 distinct
                    alleles of about 60 bases: repeats of the site's motif, a few of equal length that differ in one base
  pathogenic loci   200 sites x 1 000 entries x (REF + 1 ALT), REF and ALTs of 1 000 to 10 000 bases, the ALTs from about 30 distinct ones
Every record carries its own bytes in the blob, as a reader of N files would hand them over.  Genotypes are 0/1-style pairs.

Arms, blocking calls on one context, host clock around each (every call ends in a synchronise inside the library):
  from the host     host blob, host outputs: the upload of the blob is part of the call
  resident          the blob already in HBM, host outputs; the two kernels from trgt_merge_kernel_ms (HIP events inside the library)
  host twin         trgt_merge_exact_host on one thread, HOST_REPEATS calls
Reported: median (min .. max) of REPEATS calls after WARMUP calls, and trgt_merge_stats[3].  Then merge_hash_kernel alone, blob resident,
for several values of the per-lane / per-wave length threshold (TRGT_MERGE_LANE_MAX on developer contexts): the library's default is chosen
from these lines.  No threshold is set and no gain is claimed beyond what the file shows.  The lines are also written to the file named
by the first argument (default: profiles/merge_exact_timing.txt).  MERGE_TIMING_SCALE=<f>: sites scaled by f (default 1)."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trgt_amd import _lib, merge  # noqa: E402

WARMUP, REPEATS, HOST_REPEATS = 3, 15, 3
ACGT = np.frombuffer(b"ACGT", np.uint8)
THRESHOLDS = (0, 32, 64, 128, 256, 1024, 1 << 20)


def med(t):
    return "median %9.3f ms  (min %.3f .. max %.3f of %d)" % (statistics.median(t), min(t), max(t), len(t))


def repeat_allele(rng, motif, length):
    return np.tile(motif, length // len(motif) + 1)[:length].copy()


def cohort(n_sites, n_entries, n_alt, n_distinct, len_lo, len_hi, ref_lo, ref_hi, seed):
    rng = np.random.default_rng(seed)
    blobs, lens = [], []
    for _ in range(n_sites):
        motif = ACGT[rng.integers(0, 4, int(rng.integers(2, 7)))]
        pool = []
        for k in range(n_distinct):
            if k and rng.random() < 0.3:      # the length of an earlier one, one base changed: decided only in the bytes
                a = pool[int(rng.integers(0, k))].copy()
                a[int(rng.integers(len(a) // 2, len(a)))] = ACGT[int(rng.integers(0, 4))]
            else:
                a = repeat_allele(rng, motif, int(rng.integers(len_lo, len_hi + 1)))
            pool.append(a)
        pool.append(repeat_allele(rng, motif, int(rng.integers(ref_lo, ref_hi + 1))))   # the REF
        w = 1.0 / np.arange(1, n_distinct + 1)
        pick = rng.choice(n_distinct, size=(n_entries, n_alt), p=w / w.sum())
        idx = np.concatenate([np.full((n_entries, 1), n_distinct), pick], axis=1).ravel()
        plen = np.array([len(a) for a in pool], np.uint32)
        lens.append(plen[idx])
        blobs.append(np.concatenate([pool[i] for i in idx]))
    allele_len = np.concatenate(lens)
    blob = np.concatenate(blobs)
    na, ne = len(allele_len), n_sites * n_entries
    off = np.zeros(na, np.uint64)
    off[1:] = np.cumsum(allele_len[:-1], dtype=np.uint64)
    per = 1 + n_alt
    gt = np.tile(np.array([(1 + 1) << 1, (min(2, n_alt) + 1) << 1], np.int32), ne)
    u64 = lambda a: np.asarray(a, np.uint64)  # noqa: E731
    return dict(n_sites=n_sites, site_entry_begin=u64(np.arange(n_sites + 1) * n_entries), entry_allele_begin=u64(np.arange(ne + 1) * per),
                entry_gt_begin=u64(np.arange(ne + 1) * 2), out_allele_begin=u64(np.arange(n_sites + 1) * (1 + n_alt * n_entries)),
                allele_off=off, allele_len=allele_len, allele_blob=blob, blob_len=len(blob), gt=gt, n_alleles=na, n_gt=len(gt))


def timed(f, n, warmup):
    t = []
    for i in range(warmup + n):
        t0 = time.perf_counter()
        f()
        if i >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    import torch
    scale = float(os.environ.get("MERGE_TIMING_SCALE", "1"))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merge_exact_timing.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("python tools/merge_exact_timing.py -- device: %s; %d calls per arm after %d warm-up calls (host twin: %d calls, one thread); site limit %d" % (
        torch.cuda.get_device_name(0), REPEATS, WARMUP, HOST_REPEATS, merge.site_alleles_limit()))
    ctx = _lib.Context(0)
    ctx.timing_enable(True)
    cohorts = (("STR catalog", dict(n_sites=max(1, int(2000 * scale)), n_entries=1000, n_alt=2, n_distinct=20, len_lo=45, len_hi=75, ref_lo=45, ref_hi=75, seed=11)),
               ("pathogenic loci", dict(n_sites=max(1, int(200 * scale)), n_entries=1000, n_alt=1, n_distinct=30, len_lo=1000, len_hi=10000, ref_lo=1000, ref_hi=10000, seed=12)))
    for name, kw in cohorts:
        b = cohort(**kw)
        outs = merge.alloc_outputs(b)
        d_blob = torch.from_numpy(b["allele_blob"]).cuda()
        say("%s: %d sites x %d entries x (REF + %d ALT), %d alleles of %d..%d bases, blob %.1f MB" % (
            name, kw["n_sites"], kw["n_entries"], kw["n_alt"], b["n_alleles"], int(b["allele_len"].min()), int(b["allele_len"].max()), b["blob_len"] / 1e6))
        t_host_blob = timed(lambda: merge.call(b, outs, ctx), REPEATS, WARMUP)
        k0, k1 = [], []

        def resident():
            merge.call(b, outs, ctx, blob=d_blob)
            ms = merge.kernel_ms(ctx)
            k0.append(ms[0]); k1.append(ms[1])
        t_res = timed(resident, REPEATS, WARMUP)
        stats = ctx.merge_stats()
        dev = {k: v.copy() for k, v in outs.items()}
        t_twin = timed(lambda: merge.call(b, outs, None), HOST_REPEATS, 0)
        same = all(np.array_equal(dev[k], outs[k]) for k in ("site_status", "out_n_alleles", "allele_map", "gt_out"))
        n_out = int(outs["out_n_alleles"].sum())
        say("  trgt_merge_exact_batch, blob from the host   %s" % med(t_host_blob))
        say("  trgt_merge_exact_batch, blob resident in HBM %s   stats %s; %d merged alleles; equal to the host twin: %s" % (med(t_res), stats, n_out, same))
        say("    merge_hash_kernel                          %s" % med(k0[WARMUP:]))
        say("    merge_site_kernel                          %s" % med(k1[WARMUP:]))
        say("  trgt_merge_exact_host, one thread            %s   (for orientation only)" % med(t_twin))
        for thr in THRESHOLDS:
            c2 = _lib.context_with_env(TRGT_MERGE_LANE_MAX=thr)
            c2.timing_enable(True)
            h = []

            def one():
                merge.call(b, outs, c2, blob=d_blob)
                h.append(merge.kernel_ms(c2)[0])
            timed(one, REPEATS, WARMUP)
            c2.close()
            say("    merge_hash_kernel, one allele per lane up to %7d bytes  %s" % (thr, med(h[WARMUP:])))
        del d_blob
    say("chosen: one allele per lane up to %d bytes (trgt_knobs::merge_lane_max, csrc/common.hpp)" % 256)
    ctx.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
