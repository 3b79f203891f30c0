"""Loci for the haplotype-tag branch of genotype_flank behind the one-wave cluster chain (trgt_amd/csrc/locus_cluster_flank.hpp): builders,
so that what a case is meant to exercise can be checked with the oracle alone (tests/test_flank_cluster_cases.py, no GPU) before
tests/test_flank_cluster_gpu.py runs it.  Every locus has genotyper="cluster", 250-base flanks and exact or mutated CAG / CCG segments of
about 60 bases unless a case says otherwise.  expected_stats is what trgt_hip_flank_cluster_stats must report: computed from the oracle's
plain result (no read metadata) and a restatement of the tag rule, never taken from the library."""
from collections import Counter

import numpy as np

from helpers import mutate, rand_dna
from test_flank_device_gpu import _ref, _tag_rule, _tagged_locus
from test_flank_gpu import _phased_locus

CAG20, CAG21 = b"CAG" * 20, b"CAG" * 21
CCG18, CCG19 = b"CCG" * 18, b"CCG" * 19
CAA_CAG19 = b"CAA" + b"CAG" * 19  # as long as CAG20 and before it in byte order


def _cl(rng, segs, hp, **kw):
    return _tagged_locus(rng, segs, hp, genotyper="cluster", **kw)


def _het(rng, n, a=CAG20, b=CAG21, hp=None, **kw):
    """every other read carries a / b; hp: the tags (default: all tagged by allele)"""
    return _cl(rng, [a if i % 2 == 0 else b for i in range(n)], hp if hp is not None else [i % 2 + 1 for i in range(n)], **kw)


# ---- what the route does with a locus, from the oracle's plain result

def route(L, q):
    """None: the route leaves the locus alone.  Else (assignment of the kept reads, frequency of the winning sequence of either group)."""
    if L.get("genotyper") != "cluster" or L.get("hp_tag") is None or len(L["reads"]) > 256:
        return None
    if q["n_alleles"] != 2 or abs(len(q["alleles"][0]) - len(q["alleles"][1])) > 10:
        return None
    kept = [int(r) for r in q["kept_read"]]
    asg, ok = _tag_rule([L["hp_tag"][r] for r in kept])
    if not ok:
        return None
    segs = [L["reads"][r][int(q["span_start"][r]):int(q["span_end"][r])] for r in kept]
    freq = [max(Counter(s for s, a in zip(segs, asg) if a == g).values()) / asg.count(g) for g in (0, 1)]
    return asg, freq


def expected_stats(loci, plain, handed=()):
    """(settled, repaired among them, handed back) -- handed: loci on the route that the case makes the device hand back"""
    done = repaired = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        r = route(L, q)
        if r is None or l in handed:
            continue
        done += 1
        repaired += min(r[1]) < 0.5
    return (done, repaired, len(handed))


def plain_results(oracle, loci, params):
    return [_ref(oracle, L, params, meta=False) for L in loci]


# ---- the cases

def case_het():
    """[0] CAG20 / CAG21 tagged by allele: settled, nothing changes.  [1] the reference repeat is the longer allele: the flip is taken."""
    rng = np.random.default_rng(301)
    return [_het(rng, 24), _het(rng, 24, tr=CAG21)]


def case_tags_against_clusters():
    """reads 0-11 CAG20, 12-23 CAG21, tags alternate: either tag group holds both sequences at exactly 0.5 -- not below it, no repair -- and
    the alleles become 60, 60 with intervals 60-63"""
    rng = np.random.default_rng(302)
    return [_cl(rng, [CAG20] * 12 + [CAG21] * 12, [i % 2 + 1 for i in range(24)])]


def case_homozygous():
    """[0] 24 x CAG20, tags alternate.  [1] 20 x CAG20 + 3 x CAG21: small_group_is_outlier, the even / odd redo of the cluster genotyper"""
    rng = np.random.default_rng(303)
    return [_cl(rng, [CAG20] * 24, [i % 2 + 1 for i in range(24)]),
            _cl(rng, [CAG20] * 20 + [CAG21] * 3, [i % 2 + 1 for i in range(23)])]


def case_threshold():
    """20 reads: 14 tagged -- accepted, the untagged alternate; 12 tagged -- refused; all tags 1 -- one group is empty, refused.  A refused
    locus carries no mismatch offsets: it stays on the device."""
    rng = np.random.default_rng(304)
    return [_het(rng, 20, hp=[i % 2 + 1 for i in range(14)] + [None] * 6),
            _het(rng, 20, hp=[i % 2 + 1 for i in range(12)] + [None] * 8),
            _het(rng, 20, hp=[1] * 20)]


def case_no_route():
    """alleles 60 / 90; ploidy 1; one read (two equal alleles, no split); two reads (settled)"""
    rng = np.random.default_rng(305)
    return [_het(rng, 24, b=b"CAG" * 30), _het(rng, 12, ploidy=1), _het(rng, 1), _het(rng, 2)]


def case_lex_tie():
    """group 0 = A, A, B, B with A = CAG20 and B = CAA + CAG x 19: equal counts, equal lengths, B first in byte order -- in both read
    orders; group 1 = 4 x CAG21"""
    rng = np.random.default_rng(306)
    A, B = CAG20, CAA_CAG19
    return [_cl(rng, g0 + [CAG21] * 4, [1] * 4 + [2] * 4) for g0 in ([A, A, B, B], [B, B, A, A])]


def case_median_tie():
    """group 0: lengths 57, 60, 63, 66, every sequence once (0.25: repaired; median 61.5 -> 61, 60 is closest); group 1: 60, 63"""
    rng = np.random.default_rng(307)
    return [_cl(rng, [b"CAG" * 19, CAG20, CAG21, b"CAG" * 22, CAG20, CAG21], [1] * 4 + [2] * 2)]


def case_noisy(seed=400):
    """12 + 12 reads of CCG x 18 / CCG x 19 with 3 % errors: no sequence reaches 0.17 in its group, both groups are repaired"""
    rng = np.random.default_rng(seed)
    segs = [mutate(rng, CCG18 if i % 2 == 0 else CCG19, 0.03, 0.015, 0.015) for i in range(24)]
    return [_cl(rng, segs, [i % 2 + 1 for i in range(24)], tr=b"CCG" * 10, motifs=(b"CCG",))]


def case_no_room():
    """12 + 12 reads of CCG x 18 / CCG x 19, every read with one substitution of its own: all sequences distinct (both tag groups are
    repaired), every segment 54 or 57 bases long, which bounds what a consensus round takes from the arenas"""
    rng = np.random.default_rng(410)
    segs = []
    for i in range(24):
        s = bytearray(CCG18 if i % 2 == 0 else CCG19)
        s[3 * (i // 2) + 1] = ord("T")
        segs.append(bytes(s))
    return [_cl(rng, segs, [i % 2 + 1 for i in range(24)], tr=b"CCG" * 10, motifs=(b"CCG",))]


def case_100_reads():
    """every fifth read untagged (80 %): the instantiation for more than 64 reads"""
    rng = np.random.default_rng(308)
    return [_het(rng, 100, hp=[None if i % 5 == 4 else i % 2 + 1 for i in range(100)])]


def case_256_reads():
    """256 candidate reads; the default max_depth keeps 250"""
    rng = np.random.default_rng(309)
    return [_het(rng, 256)]


def case_long_segments():
    """6 + 6 reads of CAG x 400 / CAG x 401 with 0.5 % errors: all distinct, both groups repaired, segments of about 1 200 bases"""
    rng = np.random.default_rng(310)
    segs = [mutate(rng, b"CAG" * (400 + i % 2), 0.003, 0.001, 0.001) for i in range(12)]
    return [_cl(rng, segs, [i % 2 + 1 for i in range(12)])]


def case_purity():
    """min_read_qual = 0.5: every tenth read has rq 0.7 and a degraded repeat (scored and possibly dropped by filter_impure_trs)"""
    rng = np.random.default_rng(311)
    loci = []
    for n in (20, 30, 70):
        segs = [(CAG20 if i % 2 == 0 else CAG21) if i % 10 != 3 else rand_dna(rng, 20) + b"CAG" * 13 for i in range(n)]
        loci.append(_cl(rng, segs, [i % 2 + 1 for i in range(n)], read_qual=[0.7 if i % 10 == 3 else 0.99 for i in range(n)]))
    return loci


RANDOM_SEED = 21


def case_random(seed=RANDOM_SEED):
    """case_random of tests/test_flank_device_gpu.py with the cluster genotyper"""
    rng = np.random.default_rng(seed)
    loci = []
    for _ in range(40):
        m = rand_dna(rng, int(rng.integers(2, 7)))
        c1 = int(rng.integers(5, 40))
        c2 = max(3, c1 + int(rng.integers(-4, 5)))
        loci.append(_phased_locus(rng, m, c1, c2, n=int(rng.integers(6, 40)), hp_frac=float(rng.choice([0.6, 0.75, 0.9, 1.0])),
                                  snv=bool(rng.integers(0, 2)), err=float(rng.choice([0.002, 0.01, 0.03])), genotyper="cluster"))
    return loci


def case_mixed():
    """size and cluster loci in one call; [3] a cluster locus without tags whose flank SNVs split it (the SNV branch, host); [5] a cluster
    locus of 300 reads (host, or the deep chain on a context set with set_cluster_max_reads: not this route's either way)"""
    rng = np.random.default_rng(312)
    size = lambda n, **kw: dict(_het(rng, n, **kw), genotyper="size")
    return [size(24), _het(rng, 24), size(18, a=CAG20, b=CAG20), _phased_locus(rng, b"CAG", 20, 21, hp_frac=0.0, snv=True, genotyper="cluster"),
            _het(rng, 16, a=CAG21, b=CAG20), _het(rng, 300), size(12, ploidy=1)]
