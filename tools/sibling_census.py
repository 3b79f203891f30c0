#!/usr/bin/env python
"""sibling_census.py [--configs 2,4] [--loci N]: on the host (trgt_synth_generate and numpy, no GPU), what the exactly found sibling
leaves the missed flank pieces of the bench batches ("sibling rule").

For every read both flank pieces are searched exactly (the leftmost occurrence, as flank_scan_wide_kernel does).  A missed piece is a
fallback job; it is an EXPENSIVE one when its read is shorter than heavy_read_len of its locus (wfa_host.hpp: the longest read of the
locus minus 1.2 flank lengths).  Where the other piece of the read was found exactly, at p, the missed piece's alignment can count only
inside the admissible region Adm -- [p + F, n) for a missed right piece, [0, p) for a missed left one -- and the table gives |Adm|
among the expensive jobs: below min_matches (the scan's drop rule), below F, then by the number of 256-diagonal strips of
F + |Adm| + 1 diagonals a pre-filter run over Adm alone would walk, next to the strips of the whole read it walks today.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import synth  # noqa: E402


def census(config, n_loci, F=250, frac=0.7):
    b = synth.generate(n_loci, first_locus=0, config=config)
    min_matches = int(math.ceil(F * frac))
    blob, flank = b["read_blob"].tobytes(), b["flank_blob"].tobytes()
    jobs = dict(all=0, heavy=0, heavy_sibling=0, light=0, light_sibling=0, light_drop=0)
    hist = dict(drop=0, below_F=0)
    strips_adm, strips_now, strips_now_all = {}, {}, 0
    for l in range(n_loci):
        a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        lo = int(b["lf_off"][l]) + int(b["lf_len"][l]) - F
        pieces = (flank[lo:lo + F], flank[int(b["rf_off"][l]):int(b["rf_off"][l]) + F])
        lens = b["read_len"][a0:a1].astype(np.int64)
        heavy_len = max(int(lens.max()) - (F + F // 5), 0) if a1 > a0 else 0
        for r in range(a0, a1):
            off, n = int(b["read_off"][r]), int(b["read_len"][r])
            read = blob[off:off + n]
            pos = [read.find(pieces[0]), read.find(pieces[1])]
            for side in (0, 1):
                if pos[side] >= 0:
                    continue
                jobs["all"] += 1
                sib = pos[side ^ 1]
                adm = None if sib < 0 else (n - sib - F if side else sib)
                if n >= heavy_len:
                    jobs["light"] += 1
                    jobs["light_sibling"] += adm is not None
                    jobs["light_drop"] += adm is not None and adm < min_matches
                    continue
                jobs["heavy"] += 1
                now = (F + n + 1 + 255) // 256
                strips_now_all += now
                if adm is None:
                    continue
                jobs["heavy_sibling"] += 1
                if adm < min_matches:
                    hist["drop"] += 1
                    continue
                if adm < F:
                    hist["below_F"] += 1
                k = (F + max(adm, F) + 1 + 255) // 256
                strips_adm[k] = strips_adm.get(k, 0) + 1
                strips_now[k] = strips_now.get(k, 0) + now
    return dict(config=config, n_loci=n_loci, n_reads=int(b["n_reads"]), min_matches=min_matches, jobs=jobs, hist=hist, strips_adm=strips_adm,
                strips_now=strips_now, strips_now_all=strips_now_all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--loci", type=int, default=10000)
    a = ap.parse_args()
    for cfg in (int(v) for v in a.configs.split(",")):
        c = census(cfg, a.loci)
        j, h = c["jobs"], c["hist"]
        pct = lambda x, of: "%5.1f %%" % (100.0 * x / of) if of else "    -"
        print("cfg%d: %d loci, %d reads, F = 250, min_matches = %d" % (cfg, c["n_loci"], c["n_reads"], c["min_matches"]))
        print("  fallback jobs %d: expensive (read < heavy_read_len) %d, others %d (sibling exact %d, of those |Adm| < min_matches %d)"
              % (j["all"], j["heavy"], j["light"], j["light_sibling"], j["light_drop"]))
        print("  expensive jobs with an exactly found sibling: %d (%s)" % (j["heavy_sibling"], pct(j["heavy_sibling"], j["heavy"])))
        print("    |Adm| < min_matches (dropped by the scan):   %6d  %s of the expensive jobs" % (h["drop"], pct(h["drop"], j["heavy"])))
        print("    min_matches <= |Adm| < F (window widened to F): %4d  %s" % (h["below_F"], pct(h["below_F"], j["heavy"])))
        for k in sorted(c["strips_adm"]):
            n = c["strips_adm"][k]
            print("    %d strips of F + max(|Adm|, F) + 1 diagonals:     %6d  %s  (whole read today: %.2f strips on average)"
                  % (k, n, pct(n, j["heavy"]), c["strips_now"][k] / n))
        left = j["heavy"] - j["heavy_sibling"]
        print("    no exact sibling (judged on the whole read):   %6d  %s" % (left, pct(left, j["heavy"])))
        print("  strips summed over the expensive jobs, whole reads: %d (%.2f per job)" % (c["strips_now_all"], c["strips_now_all"] / max(j["heavy"], 1)))


if __name__ == "__main__":
    main()
