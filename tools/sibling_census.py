#!/usr/bin/env python
"""sibling_census.py [--configs 2,4] [--loci N]: on the host (trgt_synth_generate and numpy, no GPU), what the exactly found sibling
leaves the missed flank pieces of the bench batches ("sibling rule").

For every read both flank pieces are searched exactly (the leftmost occurrence, as flank_scan_wide_kernel does).  A missed piece is a
fallback job; it is an EXPENSIVE one when its read is shorter than heavy_read_len of its locus (wfa_host.hpp: the longest read of the
locus minus 1.2 flank lengths).  Where the other piece of the read was found exactly, at p, the missed piece's alignment can count only
inside the admissible region Adm -- [p + F, n) for a missed right piece, [0, p) for a missed left one -- and the table gives |Adm|
among the expensive jobs: below min_matches (the scan's drop rule), below F, then by the number of 256-diagonal strips of
F + |Adm| + 1 diagonals a pre-filter run over Adm alone would walk, next to the strips of the whole read it walks today.

The expensive jobs the scan does emit then meet the front seed search (flank_window_kernel), restated here as front_search(): settled
by a shortcut (one or two substitutions on one diagonal, one inserted or deleted base), windowed, or left without seeds for the
pre-filter.  The last rows count the jobs without seeds whose sibling is settled by a shortcut and leaves them fewer than min_matches
bases -- what settled_sibling_kernel drops, to hold the device's TRGT_WFA_DEBUG count against (reads beyond the dedicated kernels' text
length, which the device keeps on a list of their own, are not modelled: a few dozen jobs on cfg4, none on cfg2).

The common-subsequence rule (lcs_rule_kernel) then looks at the jobs without seeds that are left beside a sibling whose span is known --
found exactly, or settled by a shortcut: an alignment of the missed piece that stays inside Adm has at most LCS(piece, read[Adm])
matches, so with LCS < min_matches the read has no span.  lcs_bound() / lcs_rule_drops() restate it (Python integers as bit vectors,
bytes outside ACGT match everything, |Adm| <= LCS_MAX_ADM); the rows give what it certifies beside either kind of sibling, the share of
the jobs without seeds and of their strips, the certified jobs by |Adm| WITHOUT the cap (what LCS_MAX_ADM was chosen from), and what the
same bound would certify among the light jobs (not built).
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import synth  # noqa: E402


def seed_plan(F, x, o, e, segments=8):
    """what span_plan (spans.hip) decides for the seed search of F-base pieces under penalties x, o, e: segment length, the bound on the
    spread of the seeded diagonals, and which shortcuts exist (hamming_max substitutions; the one-base gap under 2,5,1 only)"""
    q = F // segments
    ok = q >= 12 and x >= 1 and e >= 1 and o >= 0 and q * e >= x and o + 2 * e >= 2 * x and o + e >= x
    s0 = x * segments - 1
    G = (s0 - o) // e if s0 >= o + e else 0
    hamming_max = min(segments - 1, (o + e - 1) // x, 4) if ok else 0
    return dict(ok=ok, F=F, m=segments, q=q, spread=2 * G, hamming_max=hamming_max, indel_ok=ok and (x, o, e) == (2, 5, 1) and hamming_max == 2)


def seeded_diagonals(read, piece, plan):
    """(kmin, kmax) over the occurrences in the read of the first twelve bases of every segment of the piece; None without any"""
    ks = []
    if len(read) >= 12:
        for i in range(plan["m"]):
            head, t = piece[i * plan["q"]:i * plan["q"] + 12], -1
            while True:
                t = read.find(head, t + 1)
                if t < 0:
                    break
                ks.append(t - i * plan["q"])
    return (min(ks), max(ks)) if ks else None


def front_search(read, piece, plan):
    """flank_window_kernel over one expensive job, restated: ("settled", st, en) when a shortcut names the alignment (its text span is
    [st, en)), ("window",) when the job joins the windowed launch, ("noseed",) when it goes on to the pre-filter"""
    F, n = plan["F"], len(read)
    kk = seeded_diagonals(read, piece, plan) if plan["ok"] else None
    if kk is None:
        return ("noseed",)
    kmin, kmax = kk
    if plan["hamming_max"] > 0 and kmin == kmax and kmin >= 0 and kmin + F <= n:  # one or two substitutions on the one seeded diagonal
        d = sum(a != b for a, b in zip(piece, read[kmin:kmin + F]))
        if 1 <= d <= plan["hamming_max"]:
            return ("settled", kmin, kmin + F)
    if plan["indel_ok"] and kmax - kmin == 1 and kmin >= 0 and kmax + F <= n and F <= 255:  # one inserted or deleted base
        m0 = [piece[b] != read[kmin + b] for b in range(F)]
        m1 = [piece[b] != read[kmin + 1 + b] for b in range(F)]
        lcp = lambda m: m.index(True) if True in m else F
        sfx = lambda m: F - m[::-1].index(True) if True in m else 0
        lcp0, lcp1, sfx0, sfx1 = lcp(m0), lcp(m1), sfx(m0), sfx(m1)
        last_head = (plan["m"] - 1) * plan["q"]
        margins = sfx0 > 13 and sfx1 > 13 and lcp0 < last_head - 1 and lcp1 < last_head - 1
        ins_ok, del_ok = sfx1 <= lcp0, max(sfx0 - 1, 0) <= min(lcp1, F - 1)
        if margins and ins_ok != del_ok and sum(m0) >= 4 and sum(m1) >= 4:
            return ("settled", kmin, kmin + F + 1) if ins_ok else ("settled", kmax, kmax + F - 1)
    if kmax - kmin <= plan["spread"] and kmin >= 0 and kmax + F <= n:
        return ("window",)
    return ("noseed",)


def settled_rule_drops(read, pieces, side, plan, min_matches):
    """the rule of settled_sibling_kernel for the missed piece `side` of a read whose other piece was missed by the exact scan too:
    True when that sibling is settled by a shortcut and leaves this piece fewer than min_matches bases of the read"""
    sib = front_search(read, pieces[side ^ 1], plan)
    if sib[0] != "settled":
        return False
    return (len(read) - sib[2] if side else sib[1]) < min_matches


LCS_MAX_ADM = 352  # spans.hip: beyond this the bound certifies fewer than 1 % of what it certifies at all (cfg2)
LCS_MAX_F = 256    # the kernel's bit vector: eight dwords


def lcs_bound(piece, text):
    """length of the longest common subsequence of piece and text, bit-parallel as lcs_rule_kernel computes it: one bit per base of the
    piece, per text byte u = V & Peq[c]; V = (V + u) | (V - u); the zero bits of V are the LCS.  A byte outside ACGT, in the piece or in
    the text, matches everything (that can only raise the bound)"""
    F = len(piece)
    ones = (1 << F) - 1
    peq = {c: 0 for c in b"ACGT"}
    for i, ch in enumerate(piece):
        for c in peq:
            if ch == c or ch not in peq:
                peq[c] |= 1 << i
    v = ones
    for ch in text:
        u = v & peq.get(ch, ones)
        v = ((v + u) | (v - u)) & ones
    return F - bin(v).count("1")


def admissible(read, side, span):
    """the part of the read an alignment of the missed piece `side` can count in, beside a sibling with text span [st, en)"""
    return read[span[1]:] if side else read[:span[0]]


def lcs_rule_drops(read, piece, side, span, min_matches, cap=LCS_MAX_ADM):
    """the rule of lcs_rule_kernel for a missed piece beside a sibling whose text span (st, en) is known: True when
    min_matches <= |Adm| <= cap, the piece fits the bit vector and LCS(piece, read[Adm]) < min_matches"""
    adm = admissible(read, side, span)
    if len(piece) > LCS_MAX_F or not min_matches <= len(adm) <= cap:
        return False
    return lcs_bound(piece, adm) < min_matches


def known_sibling_span(read, pieces, side, plan):
    """((st, en), kind) of the sibling of the missed piece `side` where the device knows it without a race: "exact" (the scan found it,
    leftmost occurrence) or "settled" (the front seed search's shortcuts); (None, None) otherwise"""
    other = pieces[side ^ 1]
    p = read.find(other)
    if p >= 0:
        return (p, p + len(other)), "exact"
    sib = front_search(read, other, plan)
    return ((sib[1], sib[2]), "settled") if sib[0] == "settled" else (None, None)


def lcs_rule_job_drops(read, pieces, side, plan, min_matches, cap=LCS_MAX_ADM):
    """the rule over one job of the list without seeds: the kind of sibling ("exact" / "settled") when it drops the job, else None"""
    span, kind = known_sibling_span(read, pieces, side, plan)
    return kind if span is not None and lcs_rule_drops(read, pieces[side], side, span, min_matches, cap) else None


def census(config, n_loci, F=250, frac=0.7, scoring=(2, 5, 1)):
    b = synth.generate(n_loci, first_locus=0, config=config)
    min_matches = int(math.ceil(F * frac))
    plan = seed_plan(F, *scoring)
    front = dict(settled=0, window=0, noseed=0, noseed_drop=0, strips=0, strips_drop=0)
    lcs = dict(exact=0, settled=0, strips=0, known=0, by_adm={}, seen_by_adm={}, light_seen=0, light_cert=0)
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
                    if adm is not None and min_matches <= adm <= LCS_MAX_ADM:  # (reported, not built: the rule runs over the expensive list only)
                        lcs["light_seen"] += 1
                        lcs["light_cert"] += lcs_rule_drops(read, pieces[side], side, (sib, sib + F), min_matches)
                    continue
                jobs["heavy"] += 1
                now = (F + n + 1 + 255) // 256
                strips_now_all += now
                if adm is None or adm >= min_matches:  # a job of the front seed search
                    kind = front_search(read, pieces[side], plan)[0]
                    front[kind] += 1
                    if kind == "noseed":
                        front["strips"] += now
                        if sib < 0 and settled_rule_drops(read, pieces, side, plan, min_matches):
                            front["noseed_drop"] += 1
                            front["strips_drop"] += now
                        else:  # the jobs settled_sibling_kernel leaves: the common-subsequence rule where the sibling's span is known
                            span, sib_kind = known_sibling_span(read, pieces, side, plan)
                            if span is not None:
                                lcs["known"] += 1
                                room = len(admissible(read, side, span))
                                bin_ = room // 32 * 32
                                lcs["seen_by_adm"][bin_] = lcs["seen_by_adm"].get(bin_, 0) + 1
                                if lcs_rule_drops(read, pieces[side], side, span, min_matches, cap=1 << 30):
                                    lcs["by_adm"][bin_] = lcs["by_adm"].get(bin_, 0) + 1
                                    if room <= LCS_MAX_ADM:
                                        lcs[sib_kind] += 1
                                        lcs["strips"] += now
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
    return dict(config=config, n_loci=n_loci, n_reads=int(b["n_reads"]), min_matches=min_matches, jobs=jobs, hist=hist, front=front, lcs=lcs, strips_adm=strips_adm,
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
        f = c["front"]
        print("  front seed search over the %d expensive jobs the scan emits: settled by a shortcut %d, windowed %d, without seeds (pre-filter) %d"
              % (f["settled"] + f["window"] + f["noseed"], f["settled"], f["window"], f["noseed"]))
        print("    of those without seeds: sibling settled by a shortcut, |Adm| < min_matches (settled-sibling rule): %d (%s)"
              % (f["noseed_drop"], pct(f["noseed_drop"], f["noseed"])))
        print("    their 256-diagonal strips of the whole read: %d of %d (%s)" % (f["strips_drop"], f["strips"], pct(f["strips_drop"], f["strips"])))
        q = c["lcs"]
        cert = q["exact"] + q["settled"]
        print("    of the others, sibling span known (exact or settled): %d; LCS(piece, read[Adm]) < min_matches with |Adm| <= %d (common-subsequence rule): "
              "%d beside an exact sibling, %d beside a settled one (%s of those without seeds)" % (q["known"], LCS_MAX_ADM, q["exact"], q["settled"], pct(cert, f["noseed"])))
        print("    their 256-diagonal strips of the whole read: %d of %d (%s)" % (q["strips"], f["strips"], pct(q["strips"], f["strips"])))
        total = sum(q["by_adm"].values())
        print("    certified without the cap, by |Adm| (jobs seen / certified / share of all certified):")
        for k in sorted(q["seen_by_adm"]):
            n = q["by_adm"].get(k, 0)
            print("      %4d-%4d: %6d %6d  %s" % (k, k + 31, q["seen_by_adm"][k], n, pct(n, total)))
        print("  light jobs beside an exact sibling with min_matches <= |Adm| <= %d: %d, of those LCS < min_matches: %d (not built)" % (LCS_MAX_ADM, q["light_seen"], q["light_cert"]))
        print("  strips summed over the expensive jobs, whole reads: %d (%.2f per job)" % (c["strips_now_all"], c["strips_now_all"] / max(j["heavy"], 1)))


if __name__ == "__main__":
    main()
