"""The cases of the SNV branch of genotype_flank behind the DEEP cluster chain (trgt_hip_set_snv_cluster_deep_device; the SNV forms of
trgt_amd/csrc/locus_cluster_flank_deep.hpp: Genotyper::Cluster loci of 257 to 2 048 candidate reads on a context that also has
set_cluster_max_reads), as builders, so that their conditions can be checked on the CPU with the oracle alone
(test_snv_cluster_deep_cases.py) before the GPU compares them (test_snv_cluster_deep_gpu.py).  A case is a deep size case of
snv_deep_cases.py with genotyper="cluster"; the expectation is the plain-Python restatement of get_trs_with_clustering
(snv_split_cases.snv_trace) over the kept reads of the cluster genotyper's plain result, as snv_cluster_cases.cluster_trace does without
its 256-read cap: never taken from the library.

Every case runs at Params(max_depth=2048) unless it says otherwise."""
from collections import Counter

import numpy as np

import flank_cluster_deep_cases as fcd
import snv_deep_cases as sd
from flank_cluster_cases import plain_results  # noqa: F401  (re-exported: the tests take it from here)
from helpers import rand_dna
from snv_cluster_cases import cl
from snv_deep_cases import CEILING, DEEP, OFFS_CAP, PURITY, SHALLOW, SKIPS, TIE_FIRST, N_TIES  # noqa: F401
from snv_split_cases import CAG20, CAG21, CCG18, CCG19, DECIDED, MAX_HAPS, MAX_SNVS, UNDECIDED, het, snv_locus, snv_trace  # noqa: F401
from test_flank_device_gpu import _tag_rule
from test_flank_gpu import _phased_locus

ZERO = (0, 0, 0, 0)


# ---- the restatement

def on_deep_list(L, max_reads=CEILING):
    return L.get("genotyper") == "cluster" and SHALLOW < len(L["reads"]) <= max_reads and L.get("ploidy", 2) != 0


def close_alleles(q):
    return q["n_alleles"] == 2 and abs(len(q["alleles"][0]) - len(q["alleles"][1])) <= 10


def tags_split(L, q):
    return L.get("hp_tag") is not None and _tag_rule([L["hp_tag"][int(r)] for r in q["kept_read"]])[1]


def route(L, q, max_reads=CEILING):
    """snv_trace over the kept reads of deep cluster locus L in the order of the oracle's plain result q; None where the route does not run
    the search (not a diploid cluster locus of 257 to max_reads reads with mismatch lists and two alleles at most 10 apart by length, or
    tags that split the reads)."""
    if not on_deep_list(L, max_reads) or L.get("ploidy", 2) != 2 or L.get("mismatch_offsets") is None or not close_alleles(q) or tags_split(L, q):
        return None
    kept = [int(r) for r in q["kept_read"]]
    so, eo = L.get("start_offset"), L.get("end_offset")
    t = snv_trace([so[r] if so is not None else 0 for r in kept], [eo[r] if eo is not None else 0 for r in kept], [L["mismatch_offsets"][r] for r in kept])
    t["kept"] = kept
    return t


def kept_segments(L, q, kept):
    return [L["reads"][r][int(q["span_start"][r]):int(q["span_end"][r])] for r in kept]


def lacks_majority(L, q, t):
    """per group of the split (members: tied reads in both): it has no sequence at 50 %"""
    _, mem, _ = t["split"]
    segs = kept_segments(L, q, t["kept"])
    return tuple(max(Counter(s for s, m in zip(segs, mem) if g in m).values()) / sum(1 for m in mem if g in m) < 0.5 for g in (0, 1))


def over_a_cap(t):
    return t["in_region"] > OFFS_CAP or len(t["snvs"]) > MAX_SNVS or len(t["haps"]) > MAX_HAPS


def undecided(t):
    return t["margin"] is not None and t["margin"] <= UNDECIDED


def expected_stats(loci, plain, max_reads=CEILING, handed=()):
    """trgt_hip_snv_cluster_deep_stats after one call on a context with the setting on and cluster_max_reads = max_reads: (done, repaired
    among them, handed back for room or limits, handed back undecided).  plain: the oracle's results without read metadata; handed: loci
    on the route that the case makes the device hand back (arena room, allele_cap)."""
    done = repaired = room = und = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        t = route(L, q, max_reads)
        if t is None:
            continue
        if over_a_cap(t):
            room += 1
        elif undecided(t):
            und += 1
        elif t["split"] is None:
            continue
        elif l in handed:
            room += 1
        else:
            done += 1
            repaired += any(lacks_majority(L, q, t))
    return (done, repaired, room, und)


def tag_stats(loci, plain, max_reads=CEILING, handed=()):
    """trgt_hip_flank_cluster_deep_stats of the same call where set_flank_cluster_deep_device is on as well"""
    return fcd.expected_stats(loci, plain, max_reads, handed)


# ---- the cases

def case_default_depth():
    """257 candidate reads at the default max_depth: 250 kept"""
    rng = np.random.default_rng(601)
    return cl([het(rng, 257)])


def case_depths():
    """257 reads (one read in the second round of 256 threads), 513 and 1 025, all kept; a 256-read and a 30-read cluster locus ride along
    and stay with the one-wave chain"""
    rng = np.random.default_rng(602)
    return cl([het(rng, 257), het(rng, 513), het(rng, 1025), het(rng, 256), het(rng, 30)])


def case_skip(n):
    loci, skip = sd.case_skip(n)
    return cl(loci), skip


def case_ties():
    return cl(sd.case_ties())


def case_margin():
    return cl(sd.case_margin())


def case_repair():
    """snv_deep_cases.case_repair, and [4] a locus whose only SNV is carried by every read: the homozygous candidate wins, no split"""
    rng = np.random.default_rng(603)
    return cl(sd.case_repair() + [het(rng, 270, at=(), hom=(-200,))])


def case_snv_cap():
    return cl(sd.case_snv_cap())


def case_hap_cap():
    return cl(sd.case_hap_cap())


def case_offset_cap():
    """[0] the 2 048-read locus with 16 384 in-region occurrences: at the cap and at the ceiling of the kernels; [1] 300 reads with 16 385:
    the 150 odd reads carry the site at 85, 59 reads (19.7 %: never called) 275 offsets each, and one of those ten more --
    150 + 59 * 275 + 10 = 16 385, one called SNV"""
    rng = np.random.default_rng(604)
    at_cap = sd.case_offset_cap()[0]
    mm = [(list(range(-290, -15)) if i < 59 else []) + (list(range(-15, -5)) if i == 0 else []) + ([85] if i % 2 else []) for i in range(300)]
    assert sum(len(m) for m in mm) == OFFS_CAP + 1
    return cl([at_cap, snv_locus(rng, [CAG20 if i % 2 == 0 else CAG21 for i in range(300)], mm)])


def case_tags_and_snvs():
    return cl(sd.case_tags_and_snvs())


def case_tags_and_snvs_repaired():
    """both loci of case_repair()[0]'s kind -- [0] tagged by group (the tag branch's), [1] without tags (the SNV branch's): on a context
    with both settings they share the third consensus round of the deep list"""
    L = case_repair()[0]
    mm = L["mismatch_offsets"]
    return [dict(L, hp_tag=[1 if -120 in m else 2 for m in mm]), dict(L)]


NO_ROOM_READS, NO_ROOM_LO, NO_ROOM_HI = fcd.NO_ROOM_READS, fcd.NO_ROOM_LO, fcd.NO_ROOM_HI


def case_no_room():
    """flank_cluster_deep_cases.case_no_room with SNVs in place of tags: 257 reads of CCG x 18 (129) / CCG x 19 (128), every read with one
    substitution of its own (all sequences distinct: both groups are repaired); the odd reads carry two SNVs"""
    L = fcd.case_no_room()[0]
    n = len(L["reads"])
    return [dict(L, hp_tag=None, start_offset=[-300] * n, end_offset=[300] * n, mismatch_offsets=[[-120, 85] if i % 2 else [] for i in range(n)])]


ALLELE_CAP = 61


def case_allele_cap():
    """220 x CAG20 + 40 x CAG21: the cluster genotyper calls 60 / 60.  The CAG21 reads and twenty of the others carry the SNVs (60 of 260
    reads: called): their group's sequence is CAG21 (40 of 60), 63 bases -- beyond an allele_cap of ALLELE_CAP, which the chain's own
    alleles fit"""
    rng = np.random.default_rng(605)
    segs = [CAG20] * 220 + [CAG21] * 40
    return [snv_locus(rng, segs, [[-120, 85] if i < 20 or i >= 220 else [] for i in range(260)], genotyper="cluster")]


def case_purity():
    return cl(sd.case_purity())


MIXED_SETTING = 300


def case_mixed():
    """[0] a shallow cluster locus, [1] a shallow size locus, [2] a deep size locus, [3] a deep cluster locus (this route's), [4] a deep
    haploid cluster locus, [5] a deep cluster locus whose only SNV is homozygous, [6] a cluster locus of 301 reads: beyond a setting of 300"""
    rng = np.random.default_rng(606)
    c = lambda L: dict(L, genotyper="cluster")
    return [c(het(rng, 24)), het(rng, 24), het(rng, 280), c(het(rng, MIXED_SETTING)), c(het(rng, 280, ploidy=1)), c(het(rng, 270, at=(), hom=(-200,))),
            c(het(rng, MIXED_SETTING + 1))]


RANDOM_SEED = 41


def case_random(seed=RANDOM_SEED):
    """24 cluster loci of 257 to 600 reads from the generator of test_flank_gpu.test_random_loci_with_read_metadata, without tags"""
    rng = np.random.default_rng(seed)
    loci = []
    for _ in range(24):
        m = rand_dna(rng, int(rng.integers(2, 7)))
        c1 = int(rng.integers(8, 30))
        c2 = max(3, c1 + int(rng.integers(-3, 4)))
        loci.append(_phased_locus(rng, m, c1, c2, n=int(rng.integers(257, 601)), hp_frac=0.0, snv=bool(rng.integers(0, 4)), err=float(rng.choice([0.002, 0.01, 0.03])),
                                  genotyper="cluster"))
    return loci


def case_six_routes():
    """one locus of every route: [0] size / tags, [1] size / SNVs, [2] cluster / tags, [3] cluster / SNVs, [4] deep cluster / tags, [5] deep
    cluster / SNVs (the tags of a locus split its reads or are all absent, so each locus is one branch's)"""
    rng = np.random.default_rng(607)
    tag = lambda L: dict(L, hp_tag=[i % 2 + 1 for i in range(len(L["reads"]))])
    bare = lambda L: dict(L, hp_tag=[None] * len(L["reads"]))
    c = lambda L: dict(L, genotyper="cluster")
    return [tag(het(rng, 24)), bare(het(rng, 24)), c(tag(het(rng, 24))), c(bare(het(rng, 24))), c(tag(het(rng, 300))), c(bare(het(rng, 300)))]


def all_cases():
    """(name, loci, Params keywords) of every case"""
    out = [("default depth", case_default_depth(), {}), ("depths", case_depths(), DEEP)]
    out += [("skip %d" % n, case_skip(n)[0], DEEP) for n in SKIPS]
    out += [("ties", case_ties(), DEEP), ("margin", case_margin(), DEEP), ("repair", case_repair(), DEEP), ("snv cap", case_snv_cap(), DEEP),
            ("hap cap", case_hap_cap(), DEEP), ("offset cap", case_offset_cap(), DEEP), ("tags and snvs", case_tags_and_snvs(), DEEP),
            ("tags and snvs repaired", case_tags_and_snvs_repaired(), DEEP), ("no room", case_no_room(), DEEP), ("allele cap", case_allele_cap(), DEEP),
            ("purity", case_purity(), dict(PURITY, **DEEP)), ("mixed", case_mixed(), DEEP), ("random", case_random(), DEEP), ("six routes", case_six_routes(), DEEP)]
    return out
