"""The cases of the SNV branch of genotype_flank on the device (trgt_hip_set_snv_split_device), as builders, so that their conditions can
be checked on the CPU with the oracle alone (test_snv_split_cases.py) before the GPU compares them (test_snv_split_gpu.py) -- and a
plain-Python restatement of get_trs_with_clustering (genotype_flank.rs:78-138, with :171-290) over the kept reads of a locus, from
which the expected statistics are computed: never from the library."""
import json
import math
import os
from collections import Counter

import numpy as np

from helpers import rand_dna
from test_flank_device_gpu import L167, L168, _noisy_group, _tag_rule
from test_flank_gpu import _kat_locus, _phased_locus

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "caller_kats.json")))
CAG20, CAG21 = b"CAG" * 20, b"CAG" * 21
X60, Y60 = CAG20, b"CAG" * 19 + b"CAT"
CCG18, CCG19 = b"CCG" * 18, b"CCG" * 19
UNDECIDED, DECIDED = 1e-12, 1e-6  # relative margins: every locus of every case is at most the one or at least the other
MAX_SNVS, MAX_HAPS, OFFS_PER_READ = 64, 16, 8  # the route's limits (locus_gt.hpp: SNV_MAX_SNVS, SNV_MAX_HAPS, SNV_OFFS_PER_READ)


# ---- the restatement

def snv_trace(start, end, mismatches):
    """get_trs_with_clustering step by step.  Returns a dict with what every step found; 'split' is None (no split) or (assignment,
    membership, relative margin): assignment[i] in (0, 1), membership[i] the set of groups read i belongs to, margin =
    (top - best other) / (1 + |top|) of the candidate search."""
    n = len(start)
    t = dict(n=n, split=None, snvs=[], in_region=0, full=0, haps=[], margin=None)
    if n == 0 or not any(len(m) for m in mismatches):
        return t
    skip = int(math.floor(n * (1.0 - 0.85) + 0.5))  # f64::round of a positive value
    t["skip"] = skip
    if skip >= n:
        return t
    reg0, reg1 = sorted(start)[n - 1 - skip], sorted(end)[skip]
    t["region"] = (reg0, reg1)
    seen = Counter(o for m in mismatches for o in m if reg0 <= o <= reg1)
    t["in_region"] = sum(seen.values())
    snvs = sorted(o for o, c in seen.items() if c / n >= 0.20)
    t["snvs"] = snvs
    prof = [tuple(None if (s < start[i] or s > end[i]) else (s in mismatches[i]) for s in snvs) for i in range(n)]
    t["profiles"] = prof
    full = [p for p in prof if None not in p]
    t["full"] = len(full)
    if len(full) / n < 0.40:
        return t
    haps = sorted(set(full))
    t["haps"] = haps
    if len(haps) * (len(haps) + 1) // 2 <= 1:
        return t
    ln_match, ln_mis, ln2 = math.log(0.9), math.log(1.0 - 0.9), math.log(2.0)

    def ev(p, h):
        v = 0.0
        for a, b in zip(p, h):
            if a is not None:
                v += ln_match if a == b else ln_mis
        return v
    cands = [(haps[a], haps[b]) for a in range(len(haps)) for b in range(a, len(haps))]
    lls = []
    for h1, h2 in cands:
        ll = 0.0
        for p in prof:
            t1, t2 = ev(p, h1), ev(p, h2)
            mx = max(t1, t2)
            ll += (mx + math.log(math.exp(t1 - mx) + math.exp(t2 - mx))) - ln2
        lls.append(ll)
    top = max(lls)
    win = max(i for i, v in enumerate(lls) if v == top)  # max_by: the last maximum
    t["margin"] = margin = (top - max(v for i, v in enumerate(lls) if i != win)) / (1.0 + abs(top))
    h1, h2 = cands[win]
    t["winner"] = (h1, h2)
    if h1 == h2:
        return t
    agree = lambda p, h: sum(1 for a, b in zip(p, h) if a is not None and a == b)
    asg, mem, k = [], [], 0
    for p in prof:
        d1, d2 = agree(p, h1), agree(p, h2)
        if d1 < d2:
            asg.append(0); mem.append({0})
        elif d1 > d2:
            asg.append(1); mem.append({1})
        else:
            asg.append(k % 2); mem.append({0, 1}); k += 1
    if not all(any(g in m for m in mem) for g in (0, 1)):  # simple_consensus of an empty group: None
        return t
    t["split"] = (asg, mem, margin)
    return t


def snv_rule(start, end, mismatches):
    return snv_trace(start, end, mismatches)["split"]


def locus_trace(L, q):
    """snv_trace over the kept reads of locus L, in the order of the oracle's plain result q; None where the route does not look at the
    locus (not a diploid size locus of at most 256 reads with two sizes at most 10 apart, no mismatch lists, or tags that split)."""
    if L.get("genotyper", "size") != "size" or len(L["reads"]) > 256 or L.get("mismatch_offsets") is None:
        return None
    if q["n_alleles"] != 2 or abs(int(q["gt_size"][0]) - int(q["gt_size"][1])) > 10:
        return None
    kept = [int(r) for r in q["kept_read"]]
    if L.get("hp_tag") is not None and _tag_rule([L["hp_tag"][r] for r in kept])[1]:
        return None
    so, eo = L.get("start_offset"), L.get("end_offset")
    t = snv_trace([so[r] if so is not None else 0 for r in kept], [eo[r] if eo is not None else 0 for r in kept], [L["mismatch_offsets"][r] for r in kept])
    t["kept"] = kept
    return t


def expected_stats(loci, plain, handed=(), big=None):
    """trgt_hip_snv_split_stats after a call with the setting on.  plain: the oracle's results without read metadata; handed: loci on
    the route that the case's environment makes the device hand back (repair envelope).  big: the call runs the 256-read forms (default:
    some locus of the batch has more than 64 reads)."""
    if big is None:
        big = any(len(L["reads"]) > 64 for L in loci)
    done = repaired = room = undecided = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        t = locus_trace(L, q)
        if t is None:
            continue
        if t["in_region"] > OFFS_PER_READ * (256 if big else 64) or len(t["snvs"]) > MAX_SNVS or len(t["haps"]) > MAX_HAPS:
            room += 1
            continue
        if t["margin"] is not None and t["margin"] <= UNDECIDED:
            undecided += 1
            continue
        if t["split"] is None:
            continue
        if l in handed:
            room += 1
            continue
        asg, mem, _ = t["split"]
        segs = [L["reads"][r][int(q["span_start"][r]):int(q["span_end"][r])] for r in t["kept"]]
        done += 1
        repaired += any(max(Counter(s for s, m in zip(segs, mem) if g in m).values()) / sum(1 for m in mem if g in m) < 0.5 for g in (0, 1))
    return (done, repaired, room, undecided)


# ---- the builders

def snv_locus(rng, segs, mm, so=None, eo=None, hp=None, tr=CAG20, motifs=(b"CAG",), **kw):
    """reads = pad + left flank + segment + right flank + pad with exact segments; start_offset / end_offset / mismatch lists as given
    (default offsets: -300 / 300 for every read); a mismatch a read's offsets do not cover is dropped from its list"""
    lf, rf = rand_dna(rng, 250), rand_dna(rng, 250)
    n = len(segs)
    so = list(so) if so is not None else [-300] * n
    eo = list(eo) if eo is not None else [300] * n
    reads = [rand_dna(rng, 30) + lf + s + rf + rand_dna(rng, 30) for s in segs]
    mm = [sorted(o for o in m if so[i] <= o <= eo[i]) for i, m in enumerate(mm)]
    return dict(dict(left_flank=lf, right_flank=rf, tr=tr, motifs=list(motifs), ploidy=2, reads=reads, genotyper="size", hp_tag=list(hp) if hp is not None else None,
                     start_offset=so, end_offset=eo, mismatch_offsets=mm), **kw)


def het(rng, n, a=CAG20, b=CAG21, at=(-120, 85), hom=(-200,), **kw):
    """every other read carries a / b; the b reads carry heterozygous SNVs at `at`, every read the homozygous ones at `hom`"""
    return snv_locus(rng, [a if i % 2 == 0 else b for i in range(n)], [list(hom) + (list(at) if i % 2 else []) for i in range(n)], **kw)


def by_profiles(rng, counts, sites=(-120, 85), **kw):
    """reads by profile over two SNVs: counts of (F,F), (F,T), (T,F), (T,T) in that order of reads; segments alternate 60 / 63 bases"""
    prof = [p for p, c in zip(((0, 0), (0, 1), (1, 0), (1, 1)), counts) for _ in range(c)]
    return snv_locus(rng, [CAG20 if i % 2 == 0 else CAG21 for i in range(len(prof))], [[s for s, on in zip(sites, p) if on] for p in prof], **kw)


def case_kats():
    """the reference's own vectors: F1 is split by its SNVs, F2 (homozygous SNVs) is not"""
    rng = np.random.default_rng(4)
    return [_kat_locus(rng, k) for k in KATS["genotype_flank"]]


def case_plain():
    """[0] 20 / 21 repeats without tags: the SNVs split the reads; [1] 12 / 30 repeats: the step does not run"""
    rng = np.random.default_rng(201)
    return [_phased_locus(rng, b"CAG", 20, 21, hp_frac=0.0, snv=True), _phased_locus(rng, b"CAG", 12, 30, hp_frac=0.0, snv=True)]


def case_skip(n):
    """n reads whose start offsets are -300 - 10 i and whose end offsets are 300 + 10 i, so that with skip = round(n * (1.0 - 0.85)) the
    region is [-300 - 10 skip, 300 + 10 skip].  Four loci with one heterozygous site each: exactly at the left edge (called), one base
    outside it (no SNV, no split), exactly at the right edge, one base outside.  A skip one too small loses the sites at the edges, one
    too large gains the sites outside."""
    rng = np.random.default_rng(202 + n)
    skip = {3: 0, 10: 2, 30: 5}[n]
    so, eo = [-300 - 10 * i for i in range(n)], [300 + 10 * i for i in range(n)]
    return [het(rng, n, at=(x,), hom=(), so=so, eo=eo) for x in (-300 - 10 * skip, -301 - 10 * skip, 300 + 10 * skip, 301 + 10 * skip)], skip


def case_call_threshold():
    """20 reads; the ten b reads carry the site at -120; 4 of them the one at 85 (4.0 / 20.0 >= 0.20: called), 3 the one at 140 (not)"""
    rng = np.random.default_rng(203)
    mm = [([-120] if i % 2 else []) + ([85] if i in (1, 3, 5, 7) else []) + ([140] if i in (9, 11, 13) else []) for i in range(20)]
    return [snv_locus(rng, [CAG20 if i % 2 == 0 else CAG21 for i in range(20)], mm)]


def case_least_full():
    """The 40 % rule cannot refuse a locus that has an SNV: an SNV lies inside the region, at most skip reads start behind the region's
    start and at most skip end before its end, so at least n - 2 skip reads (14 of 20) observe every SNV.  This is that extreme: three
    reads start behind the left site, three others end before the right one."""
    rng = np.random.default_rng(204)
    so = [-100 if i in (0, 2, 4) else -300 for i in range(20)]
    eo = [50 if i in (1, 3, 5) else 300 for i in range(20)]
    return [het(rng, 20, so=so, eo=eo, hom=())]


def case_ties():
    """10 reads, skip = 2, one heterozygous site at -120.  Reads 8 and 9 start behind it: they observe nothing, agree equally with both
    haplotypes, join both groups, and their assignment alternates 0, 1.  The carriers (group 0) are W63 x 4; the others (group 1) are X60,
    X60, Y60, Y60.  The two tie reads are Y60 and a 66-base one: with both of them group 1 has Y60 three times against X60 twice --
    by assignment alone it would hold X60 x 2, Y60 x 2 and the 66-base read, and X60 (first in the order) would win -- and group 0's
    interval is (60, 66) although the reads assigned to it span (60, 63).  num_spanning is 5 / 5, the groups have 6 members each."""
    rng = np.random.default_rng(205)
    segs = [CAG21, X60, CAG21, X60, CAG21, Y60, CAG21, Y60, Y60, b"CAG" * 22]
    mm = [[-120] if s == CAG21 else [] for s in segs]
    so = [-300] * 8 + [-100, -100]
    return [snv_locus(rng, segs, mm, so=so, tr=b"CAG" * 10)]


def case_margin():
    """[0] one read of each profile over two SNVs and [1] (F,F) x 2, (T,F) x 3, (T,T) x 2: the best candidates differ in the last bits or
    not at all -- undecided, the host's; [2] three distinct profiles, (F,F) x 6, (T,F) x 1, (T,T) x 6, with a clear winner"""
    rng = np.random.default_rng(206)
    return [by_profiles(rng, (1, 1, 1, 1)), by_profiles(rng, (2, 0, 3, 2)), by_profiles(rng, (6, 0, 1, 6))]


SEED_G18, SEED_G19, SEED_SWAP = 3, 11, 5  # as in test_flank_device_gpu.case_repair


def case_repair():
    """The carriers of the SNVs are group 0 (fewer agreements with the first, all-false haplotype).  [0] both groups noisy: both
    repaired; [1] the carriers are the noisy longer group: repaired, longer than allele 1, so the alleles swap and the assignment flips;
    [2] / [3] carriers with the longer allele, clean: swap; tr = the shorter allele (first after the swap: no flip), tr = the longer
    one (second after the swap: the reference allele moves to the front)"""
    rng = np.random.default_rng(207)
    g18, g19, gsw = _noisy_group(SEED_G18, CCG18), _noisy_group(SEED_G19, CCG19), _noisy_group(SEED_SWAP, CCG19)
    kw = dict(tr=b"CCG" * 10, motifs=(b"CCG",))
    mm = [[-120, 85, -200]] * 8 + [[-200]] * 8
    return [snv_locus(rng, g18 + g19, mm, **kw), snv_locus(rng, gsw + [CCG18] * 8, mm, **kw),
            snv_locus(rng, [CAG21] * 6 + [CAG20] * 6, [[-120]] * 6 + [[]] * 6, tr=CAG20), snv_locus(rng, [CAG21] * 6 + [CAG20] * 6, [[-120]] * 6 + [[]] * 6, tr=CAG21)]


def case_hand_back():
    """a repair locus whose segments (about 70 bases) are beyond a 60-base repair envelope, next to one that needs no repair"""
    rng = np.random.default_rng(208)
    g = _noisy_group(7, b"CCG" * 23 + b"C")
    return [snv_locus(rng, g + [b"CCG" * 24] * 8, [[-120, 85]] * 8 + [[]] * 8, tr=b"CCG" * 10, motifs=(b"CCG",)), het(rng, 16)]


def case_forms():
    """100 and 256 reads: the large instantiation (a 30-read locus rides along)"""
    rng = np.random.default_rng(209)
    return [het(rng, 100), het(rng, 256), het(rng, 30)]


def case_segments_beyond_lds(n, big):
    rng = np.random.default_rng(210)
    return [het(rng, n, a=L167, b=L168)] + ([het(rng, 65)] if big else [])


def case_purity():
    """min_read_qual = 0.5: every tenth read has rq 0.7 and a degraded repeat (scored and possibly dropped by filter_impure_trs)"""
    rng = np.random.default_rng(211)
    loci = []
    for n in (20, 30, 40):
        segs = [(CAG20 if i % 2 == 0 else CAG21) if i % 10 != 3 else rand_dna(rng, 20) + b"CAG" * 13 for i in range(n)]
        loci.append(snv_locus(rng, segs, [[-200] + ([-120, 85] if i % 2 else []) for i in range(n)], read_qual=[0.7 if i % 10 == 3 else 0.99 for i in range(n)]))
    return loci


def case_snv_cap():
    """[0] 64 called SNVs (the masks are full), [1] 65.  10 reads; the five b reads carry them all (320 / 325 offsets)"""
    rng = np.random.default_rng(212)
    return [het(rng, 10, at=tuple(range(-200, -200 + 2 * k, 2)), hom=()) for k in (MAX_SNVS, MAX_SNVS + 1)]


def case_hap_cap():
    """[0] 16 distinct fully observed profiles, [1] 17: twelve reads each of the all-false and the all-true profile over five SNVs decide
    the search, 14 / 15 single reads carry the other profiles (every SNV is carried by more than 20 % of the reads)"""
    rng = np.random.default_rng(213)
    sites = (-150, -120, -90, 60, 85)
    loci = []
    for k in (MAX_HAPS, MAX_HAPS + 1):
        prof = [0] * 12 + [31] * 12 + [3, 5, 6, 9, 10, 12, 17, 18, 20, 24, 7, 11, 13, 14, 19][:k - 2]
        loci.append(snv_locus(rng, [CAG21 if bin(p).count("1") >= 3 else CAG20 for p in prof], [[s for j, s in enumerate(sites) if p >> j & 1] for p in prof]))
    return loci


def case_offset_cap(big):
    """in-region offsets at the cap of the form (8 per read slot: 512 for the 64-read forms, 2 048 for the 256-read ones) and one beyond:
    n reads (40 / 100) all carry h homozygous sites, the b reads one heterozygous site, and single reads a site of their own"""
    rng = np.random.default_rng(214)
    n, h, cap = (100, 19, 2048) if big else (40, 12, 512)
    loci = []
    for extra in (0, 1):
        lone = cap + extra - n * h - n // 2
        assert 0 <= lone <= n
        L = het(rng, n, at=(85,), hom=tuple(range(-250, -250 + 3 * h, 3)))
        for i in range(lone):
            L["mismatch_offsets"][i] = sorted(L["mismatch_offsets"][i] + [100 + i])
        loci.append(L)
    return loci


def case_tags_and_snvs():
    """[0] tags that split the reads (and SNVs that would as well): the tag branch owns the locus; [1] half of the reads tagged: the tags
    are refused and the SNVs split the reads"""
    rng = np.random.default_rng(215)
    return [het(rng, 24, hp=[i % 2 + 1 for i in range(24)]), het(rng, 24, hp=[(i % 2 + 1) if i < 12 else None for i in range(24)])]


def case_mixed():
    """size loci with a split ([0], [5], and [4], whose alleles are equal by length), a cluster locus, a 300-read locus, a haploid one
    and a size locus whose only SNV is homozygous"""
    rng = np.random.default_rng(216)
    return [het(rng, 24), _phased_locus(rng, b"AT", 25, 27, hp_frac=0.0, snv=True, genotyper="cluster"), het(rng, 300), het(rng, 12, ploidy=1),
            het(rng, 18, a=CAG20, b=CAG20), _phased_locus(rng, b"CAG", 20, 22, hp_frac=0.0, snv=True), het(rng, 16, at=(), hom=(-200,))]


RANDOM_SEED = 21


def case_random():
    """40 loci from the generator of test_flank_gpu.test_random_loci_with_read_metadata, size genotyper"""
    rng = np.random.default_rng(RANDOM_SEED)
    loci = []
    for _ in range(40):
        m = rand_dna(rng, int(rng.integers(2, 7)))
        c1 = int(rng.integers(5, 40))
        c2 = max(3, c1 + int(rng.integers(-4, 5)))
        loci.append(_phased_locus(rng, m, c1, c2, n=int(rng.integers(6, 40)), hp_frac=float(rng.choice([0.0, 0.6, 0.9, 1.0])),
                                  snv=bool(rng.integers(0, 2)), err=float(rng.choice([0.002, 0.01, 0.03]))))
    return loci


def all_cases():
    """(name, loci, params keywords) of every case"""
    out = [("kats", case_kats(), {}), ("plain", case_plain(), {})]
    out += [("skip %d" % n, case_skip(n)[0], {}) for n in (3, 10, 30)]
    out += [("call threshold", case_call_threshold(), {}), ("least full", case_least_full(), {}), ("ties", case_ties(), {}), ("margin", case_margin(), {}),
            ("repair", case_repair(), {}), ("hand back", case_hand_back(), {}), ("forms", case_forms(), {}),
            ("beyond lds small", case_segments_beyond_lds(20, False), {}), ("beyond lds big", case_segments_beyond_lds(40, True), {}),
            ("purity", case_purity(), dict(min_read_qual=0.5)), ("snv cap", case_snv_cap(), {}), ("hap cap", case_hap_cap(), {}),
            ("offset cap small", case_offset_cap(False), {}), ("offset cap big", case_offset_cap(True), {}),
            ("tags and snvs", case_tags_and_snvs(), {}), ("mixed", case_mixed(), {}), ("random", case_random(), {})]
    return out
