"""The cases of the SNV branch of genotype_flank for deep size loci (the SNV forms of the two deep size kernels, locus_gt_deep.hpp:
Genotyper::Size loci of 257 to 2 048 candidate reads on a context with trgt_hip_set_snv_split_device and trgt_hip_set_size_max_reads both
set), as builders, and what trgt_hip_snv_split_stats / trgt_hip_size_deep_stats must report, computed from the oracle's plain result and
the plain-Python restatement of get_trs_with_clustering (snv_trace of snv_split_cases.py): never from the library.  Shared by
tests/test_snv_deep_cases.py (the conditions every case claims, with the oracle alone) and tests/test_snv_deep_gpu.py (the runs).

Every case runs at Params(max_depth=2048), which keeps all reads of a locus; loci are those of snv_split_cases.py at depth: 250-base
flanks, exact 60 / 63-base segments, start_offset / end_offset -300 / 300 unless a case says otherwise."""
from collections import Counter

import numpy as np

import flank_deep_cases as fc
import snv_split_cases as sc
from helpers import rand_dna
from snv_split_cases import CAG20, CAG21, CCG18, CCG19, DECIDED, MAX_HAPS, MAX_SNVS, OFFS_PER_READ, UNDECIDED, X60, Y60, by_profiles, het, snv_locus, snv_trace
from test_flank_device_gpu import _tag_rule
from test_flank_gpu import _phased_locus

SHALLOW, CEILING = 256, 2048
DEEP = dict(max_depth=2048)
OFFS_CAP = OFFS_PER_READ * CEILING  # in-region occurrences of a deep locus: 8 per read slot of the kernel, whatever the locus' depth
W63 = CAG21


# ---- the restatement

def is_deep(L, max_reads=CEILING):
    return L.get("genotyper", "size") == "size" and SHALLOW < len(L["reads"]) <= max_reads and L.get("ploidy", 2) != 0


def close_alleles(q):
    return q["n_alleles"] == 2 and abs(int(q["gt_size"][0]) - int(q["gt_size"][1])) <= 10


def tags_split(L, q):
    return L.get("hp_tag") is not None and _tag_rule([L["hp_tag"][int(r)] for r in q["kept_read"]])[1]


def locus_trace(L, q, max_reads=CEILING):
    """snv_trace over the kept reads of deep locus L, in the order of the oracle's plain result q; None where the deep route does not look
    at the locus (not a diploid size locus of 257 to max_reads reads with two sizes at most 10 apart, no mismatch lists, or tags that split)"""
    if not is_deep(L, max_reads) or L.get("ploidy", 2) != 2 or L.get("mismatch_offsets") is None or not close_alleles(q) or tags_split(L, q):
        return None
    kept = [int(r) for r in q["kept_read"]]
    so, eo = L.get("start_offset"), L.get("end_offset")
    t = snv_trace([so[r] if so is not None else 0 for r in kept], [eo[r] if eo is not None else 0 for r in kept], [L["mismatch_offsets"][r] for r in kept])
    t["kept"] = kept
    return t


def kept_segments(L, q, kept):
    return [L["reads"][r][int(q["span_start"][r]):int(q["span_end"][r])] for r in kept]


def needs_repair(L, q, t):
    """a group of the split (members: tied reads in both) has no sequence at 50 %; returns the pair of flags"""
    _, mem, _ = t["split"]
    segs = kept_segments(L, q, t["kept"])
    return tuple(max(Counter(s for s, m in zip(segs, mem) if g in m).values()) / sum(1 for m in mem if g in m) < 0.5 for g in (0, 1))


def over_a_cap(t):
    return t["in_region"] > OFFS_CAP or len(t["snvs"]) > MAX_SNVS or len(t["haps"]) > MAX_HAPS


def expected_stats(loci, plain, max_reads=CEILING, handed=(), flank_device=False):
    """(trgt_hip_snv_split_stats, trgt_hip_size_deep_stats) after one call on a context with the SNV setting on and size_max_reads =
    max_reads.  plain: the oracle's results without read metadata; handed: loci on a route that the case's environment makes the device
    hand back (repair envelope); flank_device: trgt_hip_set_flank_device is on as well (a deep locus whose tags split is the tag
    route's).  The shallow loci of the batch count as snv_split_cases.expected_stats says."""
    snv = list(sc.expected_stats(loci, plain, handed))
    sd = [0, 0, 0, 0]
    for l, (L, q) in enumerate(zip(loci, plain)):
        if not is_deep(L, max_reads):
            continue
        t = locus_trace(L, q, max_reads)
        if t is None:
            route = fc.on_route(L, q, max_reads) if flank_device else None
            if route is not None and l in handed:
                sd[2] += 1
            elif route is not None:
                sd[0] += 1; sd[1] += route[1]
            else:
                sd[0] += 1; sd[1] += q["stats"]["n_wfa_cons"] > 0  # the length genotype, repaired or not (a tag split the host finds changes no count)
            continue
        if over_a_cap(t):
            snv[2] += 1; sd[2] += 1
        elif t["margin"] is not None and t["margin"] <= UNDECIDED:
            snv[3] += 1; sd[2] += 1
        elif t["split"] is None:
            sd[0] += 1; sd[1] += q["stats"]["n_wfa_cons"] > 0
        elif l in handed:
            snv[2] += 1; sd[2] += 1
        else:
            rep = any(needs_repair(L, q, t))
            snv[0] += 1; snv[1] += rep
            sd[0] += 1; sd[1] += rep; sd[3] += 1
    return tuple(snv), tuple(sd)


def tag_route_stats(loci, plain, max_reads=CEILING, handed=()):
    """out[0], out[1], out[3] of trgt_hip_flank_stats on a context with all three settings: what the tag route settled"""
    done = rep = deep = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        route = fc.on_route(L, q, max_reads)
        if route is not None and l not in handed:
            done += 1; rep += route[1]; deep += len(L["reads"]) > SHALLOW
    return done, rep, deep


# ---- the cases

def case_depths():
    """257 reads (one full round of 256 threads plus one), 513; the 256-read locus stays with the one-wave form, the 30-read one rides along"""
    rng = np.random.default_rng(301)
    return [het(rng, 257), het(rng, 513), het(rng, 256), het(rng, 30)]


SKIPS = {270: 41, 290: 44}  # round(n * (1.0 - 0.85)): n * 0.15000000000000002 = 40.500000000000006 and 43.50000000000001


def case_skip(n):
    """Sorted, the end offsets are ..., 280, 280, 290, 290, 300, 310, 310, 320, 320, ... with the single 300 at rank skip (and the start
    offsets their mirror image), dealt to the reads in a random order: repeated values on both sides of the selected rank, and a skip one
    too small or too large selects 290 or 310.  Four loci with one heterozygous site each: exactly at the right edge of the region (called),
    one base outside (no SNV, no split), and the same on the left."""
    rng = np.random.default_rng(302 + n)
    skip = SKIPS[n]
    g = lambda j: 0 if j == skip else (1 + (j - skip - 1) // 2 if j > skip else -1 - (skip - 1 - j) // 2)
    asc = [300 + 10 * g(j) for j in range(n)]
    eo = [asc[int(j)] for j in rng.permutation(n)]
    so = [-asc[int(j)] for j in rng.permutation(n)]
    return [het(rng, n, at=(x,), hom=(), so=so, eo=eo) for x in (300, 301, -300, -301)], skip


def case_call_threshold():
    """260 reads; [0] 52 of the b reads carry the three sites (52.0 / 260.0 >= 0.20: all called, the reads split), [1] 51 (no SNV, no
    split).  (Three sites: one site on a fifth of the reads loses the search to the homozygous candidate.)"""
    rng = np.random.default_rng(303)
    loci = []
    for c in (52, 51):
        mm = [[-150, -120, 85] if i % 2 == 1 and i < 2 * c else [] for i in range(260)]
        loci.append(snv_locus(rng, [CAG20 if i % 2 == 0 else CAG21 for i in range(260)], mm))
    return loci


def case_least_full():
    """The extreme of the 40 % rule that exists (an SNV lies inside the region, so at most skip reads start behind it and at most skip
    end before it: at least n - 2 skip reads observe every SNV).  260 reads, skip = 39: 39 reads start behind the left site, 39 others end
    before the right one, 182 are fully observed -- the fewest that still yield candidates."""
    rng = np.random.default_rng(304)
    so = [-100 if i < 78 and i % 2 == 0 else -300 for i in range(260)]
    eo = [50 if i < 78 and i % 2 == 1 else 300 for i in range(260)]
    return [het(rng, 260, so=so, eo=eo, hom=())]


TIE_FIRST, N_TIES = 253, 5  # the 254th to the 258th read of the kept list


def case_ties():
    """Three heterozygous sites.  Kept order: 258 reads of 60 bases in input order (X60 non-carriers, but the reads at kept positions
    253 .. 257 are Y60, start behind the left sites and end before the right one: they observe nothing, agree equally with both haplotypes, join both groups, and their
    assignment alternates 0, 1, 0 | 1, 0 across the boundary of the first round of 256 -- a count that starts again there gives 0, 1, 0 | 0,
    1), then 70 carriers of 63 bases: W63 x 36 and three other sequences (12, 11, 11).  The carriers are group 0: 36 of 70 by assignment
    alone, 36 of 75 with the tied reads -- below 50 %, so group 0 needs the repair because of them."""
    rng = np.random.default_rng(305)
    v63 = [b"CAG" * 20 + b"CAT", b"CAA" + b"CAG" * 20, b"CAG" * 10 + b"CCG" + b"CAG" * 10]
    ties = range(TIE_FIRST, TIE_FIRST + N_TIES)
    segs = [Y60 if i in ties else X60 for i in range(258)]
    carriers = [W63] * 36 + [v63[0]] * 12 + [v63[1]] * 11 + [v63[2]] * 11
    order = rng.permutation(len(carriers))
    segs += [carriers[int(j)] for j in order]
    mm = [[] for _ in range(258)] + [[-150, -120, 85]] * 70
    so = [-100 if i in ties else -300 for i in range(258)] + [-300] * 70
    eo = [50 if i in ties else 300 for i in range(258)] + [300] * 70
    return [snv_locus(rng, segs, mm, so=so, eo=eo, tr=b"CAG" * 10)]


def case_margin():
    """[0] 65 reads of each profile over two SNVs: an exactly tied symmetric set; [1] (F,F) x 130, (T,F) x 195, (T,T) x 130, the replicated near-tie of
    snv_split_cases.case_margin: the best candidates differ in the last bits or not at all -- both undecided, the host's; [2] (F,F) x 130, (T,F) x 10,
    (T,T) x 130 with a clear winner"""
    rng = np.random.default_rng(306)
    return [by_profiles(rng, (65, 65, 65, 65)), by_profiles(rng, (130, 0, 195, 130)), by_profiles(rng, (130, 0, 10, 130))]


def case_repair():
    """280 / 260 reads.  The carriers of the SNVs are group 0.  [0] both groups noisy: both repaired; [1] the carriers are the noisy longer
    group: repaired, longer than allele 1, so the alleles swap and the assignment flips; [2] / [3] carriers with the longer allele, clean:
    swap; tr = the shorter allele (first after the swap: no flip), tr = the longer one (the reference allele moves to the front)"""
    rng = np.random.default_rng(307)
    g18, g19, gsw = fc.noisy_group(fc.SEED_G18, CCG18, 140, 5), fc.noisy_group(fc.SEED_G19, CCG19, 140, 5), fc.noisy_group(fc.SEED_SWAP, CCG19, 140, 5)
    kw = dict(tr=b"CCG" * 10, motifs=(b"CCG",))
    mm = [[-120, 85, -200]] * 140 + [[-200]] * 140
    return [snv_locus(rng, g18 + g19, mm, **kw), snv_locus(rng, gsw + [CCG18] * 140, mm, **kw),
            snv_locus(rng, [CAG21] * 130 + [CAG20] * 130, [[-120]] * 130 + [[]] * 130, tr=CAG20), snv_locus(rng, [CAG21] * 130 + [CAG20] * 130, [[-120]] * 130 + [[]] * 130, tr=CAG21)]


def case_hand_back():
    """a deep repair locus whose segments (about 70 bases) are beyond a 60-base repair envelope, next to a deep one that needs no repair"""
    rng = np.random.default_rng(308)
    g = fc.noisy_group(7, b"CCG" * 23 + b"C", 130, 5)
    return [snv_locus(rng, g + [b"CCG" * 24] * 130, [[-120, 85]] * 130 + [[]] * 130, tr=b"CCG" * 10, motifs=(b"CCG",)), het(rng, 270)]


def case_snv_cap():
    """[0] 64 called SNVs (the masks are full), [1] 65.  260 reads; the 130 b reads carry them all"""
    rng = np.random.default_rng(309)
    return [het(rng, 260, at=tuple(range(-200, -200 + 2 * k, 2)), hom=()) for k in (MAX_SNVS, MAX_SNVS + 1)]


def case_hap_cap():
    """[0] 16 distinct fully observed profiles, [1] 17: 125 reads each of the all-false and the all-true profile over five SNVs decide the
    search, 14 / 15 single reads carry the other profiles (every SNV is carried by more than 20 % of the reads)"""
    rng = np.random.default_rng(310)
    sites = (-150, -120, -90, 60, 85)
    loci = []
    for k in (MAX_HAPS, MAX_HAPS + 1):
        prof = [0] * 125 + [31] * 125 + [3, 5, 6, 9, 10, 12, 17, 18, 20, 24, 7, 11, 13, 14, 19][:k - 2]
        loci.append(snv_locus(rng, [CAG21 if bin(p).count("1") >= 3 else CAG20 for p in prof], [[s for j, s in enumerate(sites) if p >> j & 1] for p in prof]))
    return loci


def case_offset_cap():
    """2 048 reads with eight in-region offsets each (16 384: at the cap, and the one locus at the ceiling of the kernels), then one read
    with nine (16 385).  Seven sites are carried by every read; the a reads carry one more at -120, the b reads one at 85."""
    rng = np.random.default_rng(311)
    hom = tuple(range(-250, -250 + 3 * 7, 3))
    loci = []
    for extra in (0, 1):
        mm = [list(hom) + ([85] if i % 2 else [-120]) + ([200] if extra and i == 0 else []) for i in range(CEILING)]
        loci.append(snv_locus(rng, [CAG20 if i % 2 == 0 else CAG21 for i in range(CEILING)], mm))
    return loci


def case_tags_and_snvs():
    """300 reads each.  [0] tags that split the reads (and SNVs that would as well): the tag branch owns the locus; [1] half of the reads
    tagged: the tags are refused and the SNVs split the reads; [2] no tags"""
    rng = np.random.default_rng(312)
    return [het(rng, 300, hp=[i % 2 + 1 for i in range(300)]), het(rng, 300, hp=[(i % 2 + 1) if i < 150 else None for i in range(300)]), het(rng, 300)]


MIXED_SETTING = 300


def case_mixed():
    """a shallow size locus, a cluster locus, a deep size locus, a deep haploid one, a deep locus whose alleles are equal by length, a
    deep one whose only SNV is homozygous, and one of 301 reads: beyond a setting of 300"""
    rng = np.random.default_rng(313)
    return [het(rng, 24), _phased_locus(rng, b"AT", 25, 27, hp_frac=0.0, snv=True, genotyper="cluster"), het(rng, MIXED_SETTING), het(rng, 280, ploidy=1),
            het(rng, 260, a=CAG20, b=CAG20), het(rng, 270, at=(), hom=(-200,)), het(rng, MIXED_SETTING + 1)]


PURITY = dict(min_read_qual=0.5)


def case_purity():
    """min_read_qual = 0.5: every tenth read has rq 0.7 and a degraded repeat (scored and possibly dropped by filter_impure_trs); the deep
    selection then runs in front of the purity batch"""
    rng = np.random.default_rng(314)
    loci = []
    for n in (260, 400):
        segs = [(CAG20 if i % 2 == 0 else CAG21) if i % 10 != 3 else rand_dna(rng, 20) + b"CAG" * 13 for i in range(n)]
        loci.append(snv_locus(rng, segs, [[-200] + ([-120, 85] if i % 2 else []) for i in range(n)], read_qual=[0.7 if i % 10 == 3 else 0.99 for i in range(n)]))
    return loci


RANDOM_SEED = 41


def case_random():
    """24 loci of 257 to 600 reads from the generator of test_flank_gpu.test_random_loci_with_read_metadata, without tags"""
    rng = np.random.default_rng(RANDOM_SEED)
    loci = []
    for _ in range(24):
        m = rand_dna(rng, int(rng.integers(2, 7)))
        c1 = int(rng.integers(8, 30))
        c2 = max(3, c1 + int(rng.integers(-3, 4)))
        loci.append(_phased_locus(rng, m, c1, c2, n=int(rng.integers(257, 601)), hp_frac=0.0, snv=bool(rng.integers(0, 4)), err=float(rng.choice([0.002, 0.01, 0.03]))))
    return loci


def all_cases():
    """(name, loci, Params keywords) of every case"""
    out = [("depths", case_depths(), DEEP)]
    out += [("skip %d" % n, case_skip(n)[0], DEEP) for n in SKIPS]
    out += [("call threshold", case_call_threshold(), DEEP), ("least full", case_least_full(), DEEP), ("ties", case_ties(), DEEP), ("margin", case_margin(), DEEP),
            ("repair", case_repair(), DEEP), ("hand back", case_hand_back(), DEEP), ("snv cap", case_snv_cap(), DEEP), ("hap cap", case_hap_cap(), DEEP),
            ("offset cap", case_offset_cap(), DEEP), ("tags and snvs", case_tags_and_snvs(), DEEP), ("mixed", case_mixed(), DEEP),
            ("purity", case_purity(), dict(PURITY, **DEEP)), ("random", case_random(), DEEP)]
    return out
