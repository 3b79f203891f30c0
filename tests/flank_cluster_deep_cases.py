"""Loci for the haplotype-tag branch of genotype_flank behind the DEEP cluster chain (trgt_amd/csrc/locus_cluster_flank_deep.hpp:
Genotyper::Cluster loci of 257 to 2 048 candidate reads on a context set with set_cluster_max_reads and set_flank_cluster_deep_device):
builders, so that what a case is meant to exercise can be checked with the oracle alone (tests/test_flank_cluster_deep_cases.py, no GPU)
before tests/test_flank_cluster_deep_gpu.py runs it.  Every locus is hand-made like those of flank_cluster_cases.py and
flank_deep_cases.py: genotyper="cluster", 250-base flanks, exact CAG / CCG segments of about 60 bases unless a case says otherwise.  A
locus is deep by its candidate reads; Params(max_depth=2048) keeps them all, the default (250) does not.

expected_stats is what trgt_hip_flank_cluster_deep_stats must report: computed from the oracle's plain result (no read metadata) and the
restatement of the tag rule for cluster loci of more than 256 reads, never taken from the library."""
from collections import Counter

import numpy as np

from flank_cluster_cases import plain_results  # noqa: F401  (re-exported: the tests take it from here)
from flank_deep_cases import BOUNDARY_UNTAGGED, CEILING, DEEP, PURITY, SHALLOW, W63, X60, Y60, group_counts, kept_segments, kept_tags, noisy_group, tag_rule_restart  # noqa: F401
from helpers import rand_dna
from test_flank_device_gpu import _tag_rule, _tagged_locus

CAG20, CAG21 = b"CAG" * 20, b"CAG" * 21
CCG18, CCG19 = b"CCG" * 18, b"CCG" * 19
CAA_CAG19 = b"CAA" + b"CAG" * 19  # as long as CAG20 and before it in byte order
CAG20_CA = CAG20 + b"CA"          # CAG20 is a proper prefix of it
AAG_CAG19_CA = b"AAG" + b"CAG" * 19 + b"CA"  # 62 bases, before CAG20 in byte order


def _cl(rng, segs, hp, **kw):
    return _tagged_locus(rng, segs, hp, genotyper="cluster", **kw)


def _het(rng, n, a=CAG20, b=CAG21, hp=None, **kw):
    """every other read carries a / b; hp: the tags (default: all tagged by allele)"""
    return _cl(rng, [a if i % 2 == 0 else b for i in range(n)], hp if hp is not None else [i % 2 + 1 for i in range(n)], **kw)


# ---- what the route does with a locus, from the oracle's plain result

def route(L, q, max_reads=CEILING):
    """None: the route leaves the locus alone.  Else (assignment of the kept reads, frequency of the winning sequence of either group)."""
    if L.get("genotyper") != "cluster" or L.get("hp_tag") is None or not SHALLOW < len(L["reads"]) <= max_reads or L.get("ploidy", 2) != 2:
        return None
    if q["n_alleles"] != 2 or abs(len(q["alleles"][0]) - len(q["alleles"][1])) > 10:
        return None
    asg, ok = _tag_rule(kept_tags(L, q))
    if not ok:
        return None
    return asg, [max(group_counts(L, q, asg, g).values()) / asg.count(g) for g in (0, 1)]


def expected_stats(loci, plain, max_reads=CEILING, handed=()):
    """(settled, repaired among them, handed back) -- handed: loci on the route that the case makes the device hand back"""
    done = repaired = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        r = route(L, q, max_reads)
        if r is None or l in handed:
            continue
        done += 1
        repaired += min(r[1]) < 0.5
    return (done, repaired, len(handed))


# ---- the cases: (loci, Params keywords)

def case_depths():
    """kept reads: 250 of 257 at the default max_depth (one round of the workgroup); then with all reads kept 257 (one read in the second
    round), 300, 513 and 1 025 (the fifth round)"""
    rng = np.random.default_rng(501)
    return [([_het(rng, 257)], {}), ([_het(rng, 257), _het(rng, 300), _het(rng, 513), _het(rng, 1025)], DEEP)]


def case_ceiling():
    """one exact-segment heterozygous locus of 2 048 reads"""
    rng = np.random.default_rng(502)
    return [_het(rng, CEILING)]


def case_tags_against_clusters():
    """reads 0-149 CAG20, 150-299 CAG21, tags alternate: either tag group holds both sequences at exactly 0.5 -- not below it, no repair --
    and the alleles become 60, 60 with intervals 60-63"""
    rng = np.random.default_rng(503)
    return [_cl(rng, [CAG20] * 150 + [CAG21] * 150, [i % 2 + 1 for i in range(300)])]


def case_homozygous():
    """[0] 300 x CAG20, tags alternate.  [1] 280 x CAG20 + 30 x CAG21: small_group_is_outlier, the even / odd redo of the cluster genotyper"""
    rng = np.random.default_rng(504)
    return [_cl(rng, [CAG20] * 300, [i % 2 + 1 for i in range(300)]),
            _cl(rng, [CAG20] * 280 + [CAG21] * 30, [i % 2 + 1 for i in range(310)])]


def case_threshold():
    """260 kept reads: 182 tagged (accepted: 182.0 / 260.0 >= 0.7 in f64), 181 (refused), all tagged 1 (one group is empty: refused).  A
    refused locus carries no mismatch offsets: it stays on the device."""
    rng = np.random.default_rng(505)
    by = lambda n: [i % 2 + 1 for i in range(n)]
    return [_het(rng, 260, hp=by(182) + [None] * 78), _het(rng, 260, hp=by(181) + [None] * 79), _het(rng, 260, hp=[1] * 260)]


def case_boundary():
    """flank_deep_cases.case_boundary for the cluster genotyper.  Kept order: 268 reads of 60 bases in input order, then 100 of 63.  Tag
    group 0 holds 132 X and 132 Y by tag: a tie that X, the lexicographically first, wins.  The untagged reads at kept positions 10 (X),
    70, 100 and 260 (Y) are k = 0 .. 3: group 0 gets those at 10 and 100 and stays tied (133 : 133, X).  A count that starts again at
    position 256 sends the read at 260 to group 0 as well: Y wins there."""
    rng = np.random.default_rng(506)
    segs, hp, t = [], [], 0
    for i in range(268):
        if i in BOUNDARY_UNTAGGED:
            segs.append(BOUNDARY_UNTAGGED[i]); hp.append(None)
        else:
            segs.append(X60 if t % 2 == 0 else Y60); hp.append(1); t += 1
    return [_cl(rng, segs + [W63] * 100, hp + [2] * 100, tr=b"CAG" * 10)]


def case_ties():
    """Tag group 0 of 130 or 131 reads against 130 x CAG21 in group 1:
    [0], [1] A = CAG20 and B = CAA + CAG x 19, 65 each, in both read orders: equal counts, equal lengths, B first in byte order
    [2] CAG20 and CAG20 + CA, 65 each: median 61, both at distance 1, CAG20 is a proper prefix and comes first
    [3] CAG20 and AAG + CAG x 19 + CA (62 bases), 65 each: both at distance 1; the longer one, later in kept order, is first in byte order
    [4] a60, a60, b66, b66, c61 x 26 (even size): equal top multiplicity, median 61: |60 - 61| < |66 - 61| (40 %: the group is repaired from a60)
    [5] the same and one more c61 (odd size: the median is the middle value, 61)
    [6] f63 = AAG + CAG20, a60, 65 each: median 61.5 -> 61: a60 (distance 1) beats f63 (distance 2), which sorts first"""
    rng = np.random.default_rng(507)
    a60, b66, c61 = CAG20, b"CAG" * 22, CAG20 + b"C"
    f63 = b"AAG" + CAG20
    mk = lambda g0: _cl(rng, g0 + [CAG21] * 130, [1] * len(g0) + [2] * 130, tr=b"CAG" * 10)
    return [mk([CAG20, CAA_CAG19] * 65), mk([CAA_CAG19, CAG20] * 65), mk([CAG20_CA, CAG20] * 65), mk([CAG20, AAG_CAG19_CA] * 65),
            mk([a60, a60, b66, b66, c61] * 26), mk([a60, a60, b66, b66, c61] * 26 + [c61]), mk([f63, a60] * 65)]


SEED_G18, SEED_G19 = 3, 11


def case_repair():
    """280 reads each.  [0] tag group 0 has five sequences of 28 reads (20 %: repaired in the third round), group 1 is clean; [1] both noisy"""
    rng = np.random.default_rng(508)
    g18, g19 = noisy_group(SEED_G18, CCG18, 140, 5), noisy_group(SEED_G19, CCG19, 140, 5)
    kw = dict(tr=b"CCG" * 10, motifs=(b"CCG",))
    return [_cl(rng, g18 + [CCG19] * 140, [1] * 140 + [2] * 140, **kw), _cl(rng, g18 + g19, [1] * 140 + [2] * 140, **kw)]


def case_reference_first():
    """300 reads, group 0 (tag 1) carries the longer allele: swap.  tr = the allele of group 1: no flip; tr = the allele of group 0, second
    after the swap: the reference allele moves to the front after all"""
    rng = np.random.default_rng(509)
    return [_het(rng, 300, a=CAG21, b=CAG20, tr=CAG20), _het(rng, 300, a=CAG21, b=CAG20, tr=CAG21)]


def case_purity():
    """min_read_qual = 0.5: every tenth read has rq 0.7 and a degraded repeat (scored and possibly dropped by filter_impure_trs); the deep
    selection then runs in front of the purity batch"""
    rng = np.random.default_rng(510)
    loci = []
    for n in (260, 400):
        segs = [(CAG20 if i % 2 == 0 else CAG21) if i % 10 != 3 else rand_dna(rng, 20) + b"CAG" * 13 for i in range(n)]
        loci.append(_cl(rng, segs, [i % 2 + 1 for i in range(n)], read_qual=[0.7 if i % 10 == 3 else 0.99 for i in range(n)]))
    return loci


def case_mixed():
    """size loci, shallow cluster loci and deep cluster loci in one call: [0] size, [1] shallow cluster (the one-wave route's), [2] deep
    cluster (this route's), [3] shallow cluster of 100 reads, [4] deep cluster, haploid (no route), [5] homozygous size locus, [6] deep
    cluster, alleles 60 / 90 (no route)"""
    rng = np.random.default_rng(511)
    size = lambda n, **kw: dict(_het(rng, n, **kw), genotyper="size")
    return [size(24), _het(rng, 24), _het(rng, 300), _het(rng, 100), _het(rng, 280, ploidy=1), size(18, a=CAG20, b=CAG20), _het(rng, 270, b=b"CAG" * 30)]


def case_setting_300():
    """at cluster_max_reads = 300: the 300-read locus is the deep chain's and this route's, the 301-read one the host's from the start"""
    rng = np.random.default_rng(512)
    return [_het(rng, 300), _het(rng, 301)]


def case_entry_points():
    rng = np.random.default_rng(513)
    return [_het(rng, 300), _het(rng, 24)] + case_repair()[:1] + case_reference_first()


NO_ROOM_READS, NO_ROOM_LO, NO_ROOM_HI = 257, 54, 57


def case_no_room():
    """257 reads of CCG x 18 (129, tag 1) / CCG x 19 (128, tag 2), every read with one substitution of its own: all sequences distinct (both
    tag groups are repaired), every segment 54 or 57 bases long, which bounds what a consensus round takes from the arenas"""
    rng = np.random.default_rng(514)
    segs = []
    for i in range(NO_ROOM_READS):
        s = bytearray(CCG18 if i % 2 == 0 else CCG19)
        v = i // 2  # the v-th variant of its allele: position v % len, the (v // len)-th other base
        p = v % len(s)
        s[p] = [c for c in b"ACGT" if c != s[p]][v // len(s)]
        segs.append(bytes(s))
    return [_cl(rng, segs, [i % 2 + 1 for i in range(NO_ROOM_READS)], tr=b"CCG" * 10, motifs=(b"CCG",))]
