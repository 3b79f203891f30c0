"""The cases of the SNV branch of genotype_flank behind the one-wave cluster chain (trgt_hip_set_snv_cluster_device; the SNV forms of
trgt_amd/csrc/locus_cluster_flank.hpp), as builders, so that their conditions can be checked on the CPU with the oracle alone
(test_snv_cluster_cases.py) before the GPU compares them (test_snv_cluster_gpu.py).  A cluster case is a size case of snv_split_cases.py
with genotyper="cluster"; the expectation is the plain-Python restatement of get_trs_with_clustering of that module (snv_trace) over
the kept reads of the cluster genotyper's plain result: never taken from the library."""
from collections import Counter

import numpy as np

import snv_split_cases as sc
from snv_split_cases import DECIDED, MAX_HAPS, MAX_SNVS, OFFS_PER_READ, UNDECIDED, by_profiles, het, snv_locus, snv_trace  # noqa: F401
from test_flank_device_gpu import _tag_rule

CAG20, CAG21, CCG18, CCG19 = sc.CAG20, sc.CAG21, sc.CCG18, sc.CCG19


def cl(loci):
    """the same loci for the cluster genotyper"""
    return [dict(L, genotyper="cluster") for L in loci]


# ---- the expectation

def cluster_trace(L, q):
    """snv_trace over the kept reads of locus L in the order of the oracle's plain result q; None where the route does not run the search
    (not a cluster locus of at most 256 reads with mismatch lists and two alleles at most 10 apart by length, or tags that split)."""
    if L.get("genotyper") != "cluster" or len(L["reads"]) > 256 or L.get("mismatch_offsets") is None:
        return None
    if q["n_alleles"] != 2 or abs(len(q["alleles"][0]) - len(q["alleles"][1])) > 10:
        return None
    kept = [int(r) for r in q["kept_read"]]
    if L.get("hp_tag") is not None and _tag_rule([L["hp_tag"][r] for r in kept])[1]:
        return None
    so, eo = L.get("start_offset"), L.get("end_offset")
    t = snv_trace([so[r] if so is not None else 0 for r in kept], [eo[r] if eo is not None else 0 for r in kept], [L["mismatch_offsets"][r] for r in kept])
    t["kept"] = kept
    return t


def expected_stats(loci, plain, handed=(), big=None):
    """trgt_hip_snv_cluster_stats after a call with the setting on: (done, repaired, room, undecided), by the rules of
    snv_split_cases.expected_stats.  plain: the oracle's results without read metadata; handed: loci on the route that the case makes the
    device hand back (arena room, allele_cap).  big: the call runs the 256-read forms (default: some cluster locus of at most 256 reads
    has more than 64)."""
    if big is None:
        big = any(L.get("genotyper") == "cluster" and 64 < len(L["reads"]) <= 256 for L in loci)
    done = repaired = room = undecided = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        t = cluster_trace(L, q)
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


# ---- the cases: those of snv_split_cases.py for the cluster genotyper ...

def case_kats():
    """the reference's own vectors: F1 is split by its SNVs, F2 (homozygous SNVs) is not"""
    return cl(sc.case_kats())


def case_skip(n):
    """snv_split_cases.case_skip: the site at the region's edge (called) or one base outside it (no SNV)"""
    loci, skip = sc.case_skip(n)
    return cl(loci), skip


def case_call_threshold():
    return cl(sc.case_call_threshold())


def case_least_full():
    return cl(sc.case_least_full())


def case_ties():
    """snv_split_cases.case_ties: 10 reads, two of which belong to both groups.  num_spanning is 5 / 5, the groups have 6 members each;
    group 1's winner (Y60) exists only by membership, group 0's interval is (60, 66) only by membership"""
    return cl(sc.case_ties())


def case_margin():
    """two undecided loci and one decided"""
    return cl(sc.case_margin())


def case_repair():
    """[0] both groups through the third round; [1] swap with the assignment flipped; [2] / [3] the reference allele first, either way"""
    return cl(sc.case_repair())


def case_no_room():
    """flank_cluster_cases.case_no_room with SNVs in place of tags: 12 + 12 reads of CCG x 18 / CCG x 19, every read with one substitution
    of its own (all sequences distinct: both groups are repaired), every segment 54 or 57 bases long; the odd reads carry two SNVs"""
    rng = np.random.default_rng(510)
    segs = []
    for i in range(24):
        s = bytearray(CCG18 if i % 2 == 0 else CCG19)
        s[3 * (i // 2) + 1] = ord("T")
        segs.append(bytes(s))
    return [snv_locus(rng, segs, [[-120, 85] if i % 2 else [] for i in range(24)], tr=b"CCG" * 10, motifs=(b"CCG",), genotyper="cluster")]


ALLELE_CAP = 61


def case_allele_cap():
    """20 x CAG20 + 3 x CAG21: the cluster genotyper drops the small group as outliers and calls 60 / 60.  The three CAG21 reads and two
    of the others carry the SNVs: their group's sequence is CAG21 (3 of 5), 63 bases -- beyond an allele_cap of ALLELE_CAP, which the
    chain's own alleles fit"""
    rng = np.random.default_rng(511)
    segs = [CAG20] * 20 + [CAG21] * 3
    return [snv_locus(rng, segs, [[-120, 85] if i in (0, 1, 20, 21, 22) else [] for i in range(23)], genotyper="cluster")]


def case_forms():
    """100 and 256 reads: the large instantiation (a 30-read locus rides along)"""
    return cl(sc.case_forms())


def case_segments_beyond_lds(n, big):
    """the 501 / 504-base segments of snv_split_cases.case_segments_beyond_lds"""
    return cl(sc.case_segments_beyond_lds(n, big))


def case_purity():
    """min_read_qual = 0.5: the forms that load the purity filter's lists"""
    return cl(sc.case_purity())


def case_snv_cap():
    return cl(sc.case_snv_cap())


def case_hap_cap():
    return cl(sc.case_hap_cap())


def case_offset_cap(big):
    return cl(sc.case_offset_cap(big))


def case_tags_and_snvs():
    """[0] tags that split the reads (and SNVs that would as well): the tag branch owns the locus; [1] half of the reads tagged: the tags
    are refused and the SNVs split the reads"""
    return cl(sc.case_tags_and_snvs())


def case_tags_and_snvs_repaired():
    """both loci of case_repair()[0]'s kind -- [0] tagged by group (the tag branch's), [1] without tags (the SNV branch's): on a context
    with both settings they share the third consensus round"""
    L = case_repair()[0]
    mm = L["mismatch_offsets"]
    return [dict(L, hp_tag=[1 if -120 in m else 2 for m in mm]), dict(L)]


def case_mixed():
    """[0] a size locus with a split, [1] a cluster locus with a split, [2] a 300-read cluster locus (the host's, or the deep chain's on a
    context set with set_cluster_max_reads: not this route's either way), [3] a haploid cluster locus, [4] a cluster locus whose only SNV
    is homozygous, [5] a size locus with a split, [6] a cluster locus whose alleles are 30 bases apart"""
    rng = np.random.default_rng(516)
    c = lambda L: dict(L, genotyper="cluster")
    return [het(rng, 24), c(het(rng, 24)), c(het(rng, 300)), c(het(rng, 12, ploidy=1)), c(het(rng, 16, at=(), hom=(-200,))), het(rng, 18),
            c(het(rng, 20, b=b"CAG" * 30))]


RANDOM_SEED = sc.RANDOM_SEED


def case_random():
    """the 40 random loci of snv_split_cases.case_random (seed 21) as cluster loci"""
    return cl(sc.case_random())


FAR_APART = {("plain", 1)}  # loci that are meant to have two alleles more than 10 bases apart


def all_cases():
    """(name, loci, params keywords) of every case"""
    out = [(name, cl(loci), kw) for name, loci, kw in sc.all_cases()]
    out += [("no room", case_no_room(), {}), ("allele cap", case_allele_cap(), {}), ("tags and snvs repaired", case_tags_and_snvs_repaired(), {}),
            ("mixed batch", case_mixed(), {})]
    return out
