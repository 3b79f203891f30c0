"""Case builders for the haplotype-tag route of the deep size genotyper (the FLANK forms of locus_gt_deep.hpp: Genotyper::Size loci of
257 to 2 048 candidate reads on a context with trgt_hip_set_flank_device and trgt_hip_set_size_max_reads both set), and the restatement of
what trgt_hip_flank_stats / trgt_hip_size_deep_stats must report.  Shared by tests/test_flank_deep_gpu.py (the runs) and
tests/test_flank_deep_cases.py (the conditions every case claims, checked with the oracle alone).

Loci are hand-made like those of test_flank_device_gpu.py: 250-base flanks, exact 60 - 70-base segments, start_offset / end_offset set, no
mismatches unless a case says so.  A locus is deep by its candidate reads; Params(max_depth=2048) keeps them all, the default (250) does not."""
from collections import Counter

import numpy as np

from helpers import mutate, rand_dna
from test_flank_device_gpu import CAG20, CAG21, CCG18, CCG19, _het, _ref, _tag_rule, _tagged_locus
from test_flank_gpu import _phased_locus

SHALLOW, CEILING = 256, 2048
DEEP = dict(max_depth=2048)
X60, Y60, W63 = CAG20, b"CAG" * 19 + b"CAT", CAG21


# ---- the restatement

def tag_rule_restart(tags, every):
    """_tag_rule with a deliberate mistake: the count of the untagged reads starts again at every `every`-th kept position"""
    asg, k = [], 0
    for i, h in enumerate(tags):
        if i % every == 0:
            k = 0
        if h in (1, 2):
            asg.append(h - 1)
        else:
            asg.append(k % 2)
            k += 1
    return asg


def kept_tags(L, q):
    return [L["hp_tag"][int(r)] for r in q["kept_read"]]


def kept_segments(L, q):
    return [L["reads"][int(r)][int(q["span_start"][int(r)]):int(q["span_end"][int(r)])] for r in q["kept_read"]]


def group_counts(L, q, asg, g):
    return Counter(s for s, a in zip(kept_segments(L, q), asg) if a == g)


def on_route(L, q, max_reads):
    """the tag split replaces the genotype of this locus on a context whose device genotypers take size loci of up to max_reads reads.
    q: the oracle's result without read metadata.  None, or (assignment, repaired)"""
    if L.get("genotyper", "size") != "size" or L.get("ploidy", 2) != 2 or len(L["reads"]) > max_reads or L.get("hp_tag") is None:
        return None
    if q["n_alleles"] != 2 or abs(int(q["gt_size"][0]) - int(q["gt_size"][1])) > 10:
        return None
    asg, ok = _tag_rule(kept_tags(L, q))
    if not ok:
        return None
    return asg, any(max(group_counts(L, q, asg, g).values()) / asg.count(g) < 0.5 for g in (0, 1))


def expected_stats(loci, plain, max_reads, sent=(), handed=()):
    """(trgt_hip_flank_stats, trgt_hip_size_deep_stats) after one call on a context with the flank setting on and size_max_reads =
    max_reads (256: the flank setting alone).  plain: the oracle's results without read metadata; sent: loci the case built for the SNV
    branch; handed: loci on the route that the case makes the device hand back.  Either counts only where the device genotyped the locus
    in the first place: a locus beyond max_reads is the host's from the start."""
    done = repaired = deep = back = 0
    sd = [0, 0, 0, 0]
    for l, (L, q) in enumerate(zip(loci, plain)):
        is_deep = L.get("genotyper", "size") == "size" and SHALLOW < len(L["reads"]) <= max_reads and L.get("ploidy", 2) != 0
        route = on_route(L, q, max_reads)
        back += l in sent and len(L["reads"]) <= max_reads
        if route is not None and l in handed:
            sd[2] += is_deep; back += 1
            continue
        if route is not None:
            done += 1; repaired += route[1]; deep += is_deep
            if is_deep:
                sd[0] += 1; sd[1] += route[1]
        elif is_deep:
            sd[0] += 1; sd[1] += q["stats"]["n_wfa_cons"] > 0  # the length genotype, repaired or not
    return (done, repaired, back, deep), tuple(sd)


def size_only_stats(loci, plain, max_reads):
    """trgt_hip_size_deep_stats on a context with size_max_reads alone: every deep size locus gets the length genotype on the device"""
    sd = [0, 0, 0, 0]
    for L, q in zip(loci, plain):
        if L.get("genotyper", "size") == "size" and SHALLOW < len(L["reads"]) <= max_reads and L.get("ploidy", 2) != 0:
            sd[0] += 1; sd[1] += q["stats"]["n_wfa_cons"] > 0
    return tuple(sd)


# ---- the cases: lists of (loci, Params keywords)

def case_depths():
    """kept reads: 250 of 257 at the default max_depth (one round of the workgroup); 257 (one read in the second round), 300, 513 with all
    reads kept; the 256-read locus takes the one-wave route and the 30-read one its small form, in the same call"""
    rng = np.random.default_rng(201)
    return [([_het(rng, 257)], {}),
            ([_het(rng, 257), _het(rng, 300), _het(rng, 513), _het(rng, 256), _het(rng, 30)], DEEP)]


def case_ceiling(noisy=False):
    """one locus of 2 048 reads; noisy: tag group 0 (1 024 reads) has no sequence at 50 %"""
    rng = np.random.default_rng(202)
    if not noisy:
        return [_het(rng, CEILING)]
    g0 = noisy_group(3, CCG18, CEILING // 2, 7)
    segs = [g0[i // 2] if i % 2 == 0 else CCG19 for i in range(CEILING)]
    return [_tagged_locus(rng, segs, [i % 2 + 1 for i in range(CEILING)], tr=b"CCG" * 10, motifs=(b"CCG",))]


def case_tags_against_lengths():
    """300 reads, alleles by i % 2; either tag group holds two thirds of one allele and one third of the other"""
    rng = np.random.default_rng(203)
    hp = [(1 if (i // 2) % 3 else 2) if i % 2 == 0 else (2 if (i // 2) % 3 else 1) for i in range(300)]
    return [_het(rng, 300, hp=hp)]


def case_threshold():
    """260 kept reads: 182 tagged (accepted: 182.0 / 260.0 >= 0.7 in f64), 181 (refused), all tagged 1 (one group is empty: refused),
    tags 0 and 3 are untagged (182: accepted, 181: refused)"""
    rng = np.random.default_rng(204)
    by = lambda n: [i % 2 + 1 for i in range(n)]
    return [_het(rng, 260, hp=by(182) + [None] * 78), _het(rng, 260, hp=by(181) + [None] * 79), _het(rng, 260, hp=[1] * 260),
            _het(rng, 260, hp=by(182) + [0, 3] * 39), _het(rng, 260, hp=by(181) + [3, 0] * 39 + [3])]


BOUNDARY_UNTAGGED = {10: X60, 70: Y60, 100: Y60, 260: Y60}


def case_boundary():
    """Kept order: 268 reads of 60 bases in input order, then 100 of 63.  Tag group 0 holds 132 X and 132 Y by tag: a tie that X, the
    lexicographically first, wins.  The untagged reads at kept positions 10 (X), 70, 100 and 260 (Y) are k = 0 .. 3: group 0 gets those at
    10 and 100 and stays tied (133 : 133, X).  A count that starts again at position 64 or at 256 sends the read at 260 to group 0 (and the
    one at 70 with it, or the one at 100 still): Y wins there."""
    rng = np.random.default_rng(205)
    segs, hp, t = [], [], 0
    for i in range(268):
        if i in BOUNDARY_UNTAGGED:
            segs.append(BOUNDARY_UNTAGGED[i]); hp.append(None)
        else:
            segs.append(X60 if t % 2 == 0 else Y60); hp.append(1); t += 1
    return [_tagged_locus(rng, segs + [W63] * 100, hp + [2] * 100, tr=b"CAG" * 10)]


def case_ties():
    """the three rules of test_flank_device_gpu.case_ties in tag groups of 130 reads"""
    rng = np.random.default_rng(206)
    a60, b66, c61, d63 = CAG20, b"CAG" * 22, b"CAG" * 20 + b"C", CAG21
    e60 = b"CAG" * 19 + b"CAT"
    f63 = b"AAG" + CAG20  # lexicographically before CAG20
    mk = lambda g0: _tagged_locus(rng, g0 + [d63] * 130, [1] * len(g0) + [2] * 130, tr=b"CAG" * 10)
    return [mk([a60, a60, b66, b66, c61] * 26),  # equal multiplicity, median 61: |60 - 61| < |66 - 61| (40 %: this group is repaired from a60)
            mk([e60, a60] * 65),                 # equal multiplicity, equal distance: the lexicographically first, a60
            mk([f63, a60] * 65)]                 # median 61.5 -> 61: a60 (distance 1) beats f63 (distance 2), which sorts first


def noisy_group(seed, base, n, variants):
    """n reads cycling over `variants` distinct sequences (no sequence reaches 50 % for 3 or more): `base` with 3 % errors"""
    rng = np.random.default_rng(seed)
    v = []
    while len(v) < variants:
        m = mutate(rng, base, 0.03, 0.015, 0.015)
        if m != base and m not in v:
            v.append(m)
    return [v[i % variants] for i in range(n)]


SEED_G18, SEED_G19, SEED_SWAP = 3, 11, 5  # checked on the CPU with the oracle: every locus of case_repair aligns (n_wfa_cons > 0), the third swaps


def case_repair():
    """280 reads each.  [0] group 0 repaired, group 1 clean; [1] both noisy; [2] group 0 (tag 1) is the noisy longer one: its repaired allele
    is longer than allele 1, so the alleles swap and the classification is 1 - (tag - 1) for every read (tr matches neither allele)"""
    rng = np.random.default_rng(207)
    g18, g19, gsw = noisy_group(SEED_G18, CCG18, 140, 5), noisy_group(SEED_G19, CCG19, 140, 5), noisy_group(SEED_SWAP, CCG19, 140, 5)
    kw = dict(tr=b"CCG" * 10, motifs=(b"CCG",))
    return [_tagged_locus(rng, g18 + [CCG19] * 140, [1] * 140 + [2] * 140, **kw),
            _tagged_locus(rng, g18 + g19, [1] * 140 + [2] * 140, **kw),
            _tagged_locus(rng, gsw + [CCG18] * 140, [1] * 140 + [2] * 140, **kw)]


def case_reference_first():
    """test_flank_device_gpu.case_reference_first at 300 reads: group 0 (tag 1) carries the longer allele: swap.  tr = the allele of group
    1: no flip; tr = the allele of group 0, second after the swap: the reference allele moves to the front after all"""
    rng = np.random.default_rng(208)
    return [_het(rng, 300, a=CAG21, b=CAG20, tr=CAG20), _het(rng, 300, a=CAG21, b=CAG20, tr=CAG21)]


PURITY = dict(min_read_qual=0.5)


def case_purity():
    """min_read_qual = 0.5: every tenth read has rq 0.7 and a degraded repeat (scored and possibly dropped by filter_impure_trs); the deep
    selection then runs in front of the purity batch"""
    rng = np.random.default_rng(209)
    loci = []
    for n in (260, 400):
        segs = [(CAG20 if i % 2 == 0 else CAG21) if i % 10 != 3 else rand_dna(rng, 20) + b"CAG" * 13 for i in range(n)]
        loci.append(_tagged_locus(rng, segs, [i % 2 + 1 for i in range(n)], read_qual=[0.7 if i % 10 == 3 else 0.99 for i in range(n)]))
    return loci


def case_hand_back():
    """a deep repair locus whose segments (70 bases) are beyond a 60-base repair envelope, next to a deep locus that needs no repair"""
    rng = np.random.default_rng(210)
    g = noisy_group(7, b"CCG" * 23 + b"C", 130, 5)
    return [_tagged_locus(rng, g + [b"CCG" * 24] * 130, [1] * 130 + [2] * 130, tr=b"CCG" * 10, motifs=(b"CCG",)), _het(rng, 270)]


def case_mixed(limit=CEILING):
    """(loci, loci sent for the SNV branch): deep and shallow tagged size loci, a haploid deep locus, a deep cluster locus, two deep loci
    without tags but with flank SNVs, and a locus of limit + 1 reads (the host's from the start)"""
    rng = np.random.default_rng(211)
    loci = [_het(rng, 300), _het(rng, 24), _het(rng, 280, ploidy=1), _phased_locus(rng, b"AT", 25, 27, n=270, hp_frac=0.0, genotyper="cluster"),
            _phased_locus(rng, b"CAG", 20, 21, hp_frac=0.0, snv=True, n=300), _phased_locus(rng, b"CAG", 20, 22, hp_frac=0.0, snv=True, n=300),
            _het(rng, 260, a=CAG20, b=CAG20), _het(rng, limit + 1)]
    return loci, (4, 5)


def case_setting_300():
    rng = np.random.default_rng(212)
    return [_het(rng, 300), _het(rng, 301)]


def case_entry_points():
    rng = np.random.default_rng(213)
    return [_het(rng, 300), _het(rng, 24)] + case_repair()[:1] + case_reference_first()


RANDOM_SEED = 31  # chosen so that the oracle alone meets the floors of test_flank_deep_cases.py


def case_random():
    """12 loci, n in 257 .. 400; the second half runs at max_depth = 2048"""
    rng = np.random.default_rng(RANDOM_SEED)
    loci = []
    for _ in range(12):
        m = rand_dna(rng, int(rng.integers(2, 7)))
        c1 = int(rng.integers(8, 30))
        c2 = max(3, c1 + int(rng.integers(-3, 4)))
        loci.append(_phased_locus(rng, m, c1, c2, n=int(rng.integers(257, 401)), hp_frac=float(rng.choice([0.6, 0.75, 0.9, 1.0])),
                                  snv=bool(rng.integers(0, 2)), err=float(rng.choice([0.002, 0.01, 0.03]))))
    return [(loci[:6], {}), (loci[6:], DEEP)]


def oracle_pair(oracle, loci, params):
    """(with read metadata: the expected result; without: what the statistics are restated from)"""
    return [_ref(oracle, L, params) for L in loci], [_ref(oracle, L, params, meta=False) for L in loci]
