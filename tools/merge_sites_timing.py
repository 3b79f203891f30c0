"""Call time of trgt_merge_sites_batch on four synthetic contigs sized like those of tools/merge_exact_timing.py, so that
the two calls of the merge path can be read side by side.

  (a) 1 000 single-sample files x 2 000 sites, every file at every site, REF + 2 ALTs of about 60 bases, no pre-1.0 file
  (b) the same with every site in 300 of the files
  (c) shape (a) with every file pre-1.0: every record is padded, the whole blob is rewritten
  (d) 200 sites, REF + 1 ALT of 1 to 10 kb, every file pre-1.0
Records are handed over file after file, as a reader of N files has them; alleles come from tools/merge_exact_timing.py's cohort().

Arms, blocking calls on one context, host clock around each (every call ends in a synchronise inside the library):
  from the host     input blob on the host, every output on the host (with a pre-1.0 file: the output blob comes back too)
  resident          input blob in HBM, output blob in HBM, rows and site arrays on the host; the three kernel groups of
                    trgt_merge_sites_kernel_ms (HIP events inside the library)
  host twin         trgt_merge_sites_host on one thread, HOST_REPEATS calls
  chained           resident sites call + trgt_merge_exact_batch on the blob where it lies (what merge.merge_contig does)
  two calls         from-the-host sites call + trgt_merge_exact_batch with the blob from the host: the round trip a caller without the
                    chain pays
Reported: median (min .. max) of REPEATS calls after WARMUP calls.  The parent of this call has no such entry point: the lines stand
against the host twin and claim nothing else.  They are also written to the file named by the first argument (default:
profiles/merge_sites_timing.txt).  MERGE_TIMING_SCALE=<f>: sites scaled by f (default 1)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from merge_exact_timing import cohort, med  # noqa: E402
from trgt_amd import _lib, merge  # noqa: E402

WARMUP, REPEATS, HOST_REPEATS = 2, 15, 3


def contig(n_files, n_sites, per_site, n_alt, pre_v1, seed, **lengths):
    """the packed input (merge.pack_sites' dict) of n_files single-sample files; every site holds per_site of them"""
    rng = np.random.default_rng(seed)
    c = cohort(n_sites=n_sites, n_entries=per_site, n_alt=n_alt, seed=seed, **lengths)
    per = 1 + n_alt
    files_of = np.stack([np.sort(rng.choice(n_files, per_site, replace=False)) for _ in range(n_sites)]) if per_site < n_files else np.tile(np.arange(n_files), (n_sites, 1))
    ent_f, ent_s = files_of.ravel(), np.repeat(np.arange(n_sites), per_site)
    order = np.lexsort((ent_s, ent_f))                       # the entries file after file, positions increasing inside a file
    nr = len(order)
    site_pos = np.sort(rng.choice(200_000_000, n_sites, replace=False)).astype(np.int64)
    a_idx = (order[:, None] * per + np.arange(per)[None, :]).ravel()
    allele_len = c["allele_len"][a_idx]
    two = lambda v, t: np.ascontiguousarray(np.asarray(v).reshape(nr, 2)).astype(t).ravel()  # noqa: E731
    alt = np.minimum(2, n_alt)
    fields = dict(gt=two(np.tile([(1 + 1) << 1, (alt + 1) << 1], nr), np.int32), AL=two(allele_len.reshape(nr, per)[:, [0, per - 1]], np.int32),
                  SD=two(rng.integers(1, 60, nr * 2), np.int32), AP=two(rng.random(nr * 2), np.float32), AM=two(rng.random(nr * 2), np.float32))
    b = dict(n_files=n_files, n_samples=np.ones(n_files, np.int32), pre_v1=np.full(n_files, int(pre_v1), np.uint8), am_is_int=np.zeros(n_files, np.uint8),
             file_record_begin=np.concatenate([[0], np.cumsum(np.bincount(ent_f, minlength=n_files))]).astype(np.uint64), pos=site_pos[ent_s[order]],
             pad_base=np.full(nr, ord("C"), np.uint8), record_allele_begin=(np.arange(nr + 1) * per).astype(np.uint64), allele_off=c["allele_off"][a_idx], allele_len=allele_len,
             allele_blob=c["allele_blob"], blob_len=c["blob_len"], n_records=nr, n_alleles=nr * per, S=n_files, any_pre_v1=bool(pre_v1))
    for k, v in fields.items():
        b[k] = dict(width=np.full(nr, 2, np.uint8), begin=(np.arange(nr + 1) * 2).astype(np.uint64), values=v.view(np.uint32))
    b["blob_need"] = int(allele_len.sum()) + nr * per
    return b


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merge_sites_timing.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("python tools/merge_sites_timing.py -- device: %s; %d calls per arm after %d warm-up calls (host twin: %d calls, one thread)" % (
        torch.cuda.get_device_name(0), REPEATS, WARMUP, HOST_REPEATS))
    ctx = _lib.Context(0)
    ctx.timing_enable(True)
    short = dict(n_distinct=20, len_lo=45, len_hi=75, ref_lo=45, ref_hi=75)
    long_ = dict(n_distinct=30, len_lo=1000, len_hi=10000, ref_lo=1000, ref_hi=10000)
    ns, nl = max(1, int(2000 * scale)), max(1, int(200 * scale))
    shapes = (("(a) every file at every site", dict(n_files=1000, n_sites=ns, per_site=1000, n_alt=2, pre_v1=False, seed=21, **short)),
              ("(b) every site in 300 of the files", dict(n_files=1000, n_sites=ns, per_site=300, n_alt=2, pre_v1=False, seed=22, **short)),
              ("(c) shape (a), every file pre-1.0", dict(n_files=1000, n_sites=ns, per_site=1000, n_alt=2, pre_v1=True, seed=21, **short)),
              ("(d) alleles of 1-10 kb, every file pre-1.0", dict(n_files=1000, n_sites=nl, per_site=1000, n_alt=1, pre_v1=True, seed=24, **long_)))
    for name, kw in shapes:
        b = contig(**kw)
        n = kw["n_sites"]
        outs = merge.alloc_sites_outputs(b, n)
        d_in = torch.from_numpy(b["allele_blob"]).cuda()
        d_out = torch.empty(max(merge.sites_sizes(b, n)["allele_blob"], 1), dtype=torch.uint8, device="cuda")
        res = dict(outs, allele_blob=d_out)
        say("%s: %d files, %d sites, %d records, %d alleles of %d..%d bases, input blob %.1f MB" % (
            name, b["n_files"], n, b["n_records"], b["n_alleles"], int(b["allele_len"].min()), int(b["allele_len"].max()), b["blob_len"] / 1e6))
        t_host = timed(lambda: merge.call_sites(b, outs, n, ctx), REPEATS, WARMUP)
        groups = [[], [], []]

        def resident():
            merge.call_sites(b, res, n, ctx, blob=d_in)
            for g, v in zip(groups, merge.sites_kernel_ms(ctx)):
                g.append(v)
        t_res = timed(resident, REPEATS, WARMUP)
        stats = ctx.merge_sites_stats()
        dev = {k: np.array(v, copy=True) for k, v in outs.items() if isinstance(v, np.ndarray) and k != "allele_blob"}
        dev_blob = d_out[:res["blob_written"]].cpu().numpy()
        t_twin = timed(lambda: merge.call_sites(b, outs, n, None), HOST_REPEATS, 0)
        same = all(np.array_equal(dev[k], outs[k]) for k in dev) and np.array_equal(dev_blob, outs["allele_blob"][:outs["blob_written"]])
        say("  trgt_merge_sites_batch, blobs on the host    %s" % med(t_host))
        say("  trgt_merge_sites_batch, blobs in HBM         %s   stats %s; equal to the host twin: %s" % (med(t_res), stats, same))
        for label, g in zip(("grouping (keys, sort, heads)", "fill (rows, entries, alleles)", "blob copy"), groups):
            say("    %-42s %s" % (label, med(g[WARMUP:])))
        say("  trgt_merge_sites_host, one thread            %s" % med(t_twin))

        def chained():
            merge.call_sites(b, res, n, ctx, blob=d_in)
            b2, blob = merge.merge_in_of_sites(b, res, blob=d_in)
            merge.call(b2, merge.alloc_outputs(b2), ctx, blob=blob)

        def two_calls():
            merge.call_sites(b, outs, n, ctx)
            b2, _ = merge.merge_in_of_sites(b, outs)
            merge.call(b2, merge.alloc_outputs(b2), ctx)
        say("  chained: sites + merge_exact, blob stays in HBM   %s" % med(timed(chained, REPEATS, WARMUP)))
        say("  two calls, the blob through the host between them %s" % med(timed(two_calls, REPEATS, WARMUP)))
        del d_in, d_out, res
    ctx.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
