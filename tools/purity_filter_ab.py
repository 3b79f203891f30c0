"""A/B of filter_impure_trs on the device (trgt_amd/csrc/locus_purity.hpp) against the all-host route it replaces, on one blocking context:
the 10 000-locus cfg2 batch and the cfg4 mix, reads resident in HBM, min_read_qual = 0.5, with two read-quality settings --
  (a) 95 % of the reads at rq 0.999 and 5 % at 0.7 (few purity jobs),   (b) read_qual = None (every spanning read is scored).
Default: both routes in one process, interleaved -- two contexts created by the developer library, one with TRGT_HOST_PURITY=1 (every
locus down the host path, the routing before the filter ran on the device), one without; `--reps` timed calls each after two warm-up
calls, median and spread (min .. max) of the call time, and the routes' results compared array by array.
`--release`: one route only, through whichever library is loaded (TRGT_HIP_LIB names another build, e.g. the parent commit's, as in
tools/ab_prev_lib.sh), plus the default mode (min_read_qual = 0.98) of both batches, which must not move.
Usage: python tools/purity_filter_ab.py [--loci 10000] [--reps 7] [--release]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, locus, synth  # noqa: E402


def summary(v):
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), n=len(v))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--release", action="store_true")
    args = ap.parse_args()
    if args.release:
        routes = {"library " + os.path.basename(os.environ.get("TRGT_HIP_LIB", "libtrgt_hip.so")): _lib.Context(0)}
    else:
        routes = {"device filter": _lib.context_with_env(TRGT_HOST_PURITY=0), "host route (TRGT_HOST_PURITY=1)": _lib.context_with_env(TRGT_HOST_PURITY=1)}
    rng = np.random.default_rng(5)
    for cfg in (2, 4):
        b = synth.generate(args.loci, first_locus=0, config=cfg)
        nr = int(b["n_reads"])
        rd, fd = torch.from_numpy(b["read_blob"]).cuda(), torch.from_numpy(b["flank_blob"]).cuda()
        settings = [("rq 95% 0.999 / 5% 0.7", 0.5, np.where(rng.random(nr) < 0.95, 0.999, 0.7)), ("read_qual None", 0.5, None)]
        if args.release:  # (first: measured before the filter settings have grown any buffer)
            settings.insert(0, ("default mode (min_read_qual 0.98)", 0.98, None))
        for name, min_rq, rq in settings:
            bb = dict(b)
            bb["read_qual"] = rq
            params = locus.Params(min_read_qual=min_rq)
            times = {k: [] for k in routes}
            outs, stats = {}, {}
            for k in range(args.reps + 2):  # (two warm-up calls: buffers, pinned slabs)
                for route, ctx in routes.items():
                    t0 = time.perf_counter()
                    out = locus.run_batch(bb, params, ctx=ctx, flank_dev=fd, reads_dev=rd)
                    dt = 1e3 * (time.perf_counter() - t0)
                    if k >= 2:
                        times[route].append(dt)
                    outs[route] = out
                    stats[route] = [int(v) for v in out.stats[:24]]
            for route in routes:
                st = stats[route]
                print(json.dumps(dict(config=cfg, loci=args.loci, reads=nr, setting=name, route=route, **summary(times[route]), hmm_jobs=st[3],
                                      spanning_reads=st[2], loci_repaired_on_device=st[18], host_ms_in_call=round(st[7] / 1e6, 3))))
            first = next(iter(routes))
            for route in routes:
                for f in ("span_start", "span_end", "read_rank", "classification", "n_alleles", "allele_len", "ci", "num_spanning", "n_spans", "motif_counts"):
                    x, y = getattr(outs[first], f), getattr(outs[route], f)
                    if not np.array_equal(x, y, equal_nan=False):
                        raise SystemExit("purity_filter_ab: %s differs between the routes (cfg%d, %s)" % (f, cfg, name))
                if not np.array_equal(outs[first].purity, outs[route].purity, equal_nan=True):
                    raise SystemExit("purity_filter_ab: purity differs between the routes (cfg%d, %s)" % (cfg, name))
    print(json.dumps(dict(same_results=True)))


if __name__ == "__main__":
    main()
