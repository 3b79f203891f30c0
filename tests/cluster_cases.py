"""The matrices of the independent cluster-genotyper checks and the loci that realise them through the public API
(tests/test_cluster_independent.py holds the CPU oracle to tests/pyward.py on them, tests/test_cluster_independent_gpu.py the host path and
both device chains).  Seeded, built once per process and never changed; reads no file.

A case is a list of repeat segments.  Its matrix is what get_dist (genotype_cluster.rs:238-248) gives for every pair: the edit distance, from
a plain DP of this file's own, or the length difference where |a| * |b| > MAX_OPS.  A segment is a random backbone of 36 to 60 bases with
substitutions at sites that are at least 3 bases apart and at least 3 bases from either end, so squared distances are small integers and
almost everything ties -- the input on which the linkage's unpinned choices decide.  locus() puts the segments between random 250-base
flanks.  get_spanning_reads sorts stably by span length: among equal lengths the matrix index of a read is its position in the list, and
Case.order records the permutation where lengths differ.

answer() is the whole restated genotype of a case under a reading of the linkage's rules (pyward's parameters); the consensus of a group
of equally long segments that differ by substitutions only is the column vote of pyconsensus.repair_consensus on all-match CIGARs, which
the CPU test holds the oracle's alleles to.  That vote does not depend on which member is the backbone, so central_read's choice on the
mutated matrix shows in no result of these loci and is not part of the answer; the mutated matrix itself is compared bit for bit on the
CPU (tests/test_cluster_independent.py), and the backbone's effect on a consensus is the matter of tests/test_consensus_vote_gpu.py."""
import functools
import math
from collections import namedtuple

import numpy as np

import pyconsensus
import pyward
from helpers import rand_dna

SIZES = (3, 4, 5, 63, 64, 65, 128, 129, 255, 256, 257, 300, 330)
TR = b"CAG" * 8  # the locus's reference repeat: shorter than every segment, so no allele equals it and tr.rs:95-101 never swaps
RULES = {"ties_last": dict(ties="last"), "lw_order": dict(lw_order="alternate"), "no_keep_previous": dict(keep_previous=False)}
SIZE_CLASSES = {"lds": (3, 64), "hbm": (65, 256), "deep": (257, 330)}
ALT = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}


# ------------------------------------------------------------------------------------------------------------------ edit distances
def edit_many(A, B):
    """Levenshtein distances of the rows of A [P, la] against the rows of B [P, lb] (uint8): the textbook table, one row at a time for all
    pairs at once; the horizontal step of a row is a running minimum of cell - column."""
    P, la = A.shape
    lb = B.shape[1]
    ramp = np.arange(lb + 1, dtype=np.int32)
    prev = np.broadcast_to(ramp, (P, lb + 1)).copy()
    for i in range(1, la + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        np.minimum(prev[:, :-1] + (A[:, i - 1:i] != B), prev[:, 1:] + 1, out=cur[:, 1:])
        prev = np.minimum.accumulate(cur - ramp, axis=1) + ramp
    return prev[:, lb]


def edit_pairs(pairs):
    """{(a, b): edit distance} for the given pairs of bytes"""
    out = {}
    by_shape = {}
    for a, b in set(pairs):
        by_shape.setdefault((len(a), len(b)), []).append((a, b))
    for (la, lb), lst in by_shape.items():
        for c in range(0, len(lst), 16384):
            chunk = lst[c:c + 16384]
            A = np.frombuffer(b"".join(a for a, _ in chunk), np.uint8).reshape(len(chunk), la)
            B = np.frombuffer(b"".join(b for _, b in chunk), np.uint8).reshape(len(chunk), lb)
            for pr, v in zip(chunk, edit_many(A, B).tolist()):
                out[pr] = v
    return out


def score(a, b, table):
    """the integer under get_dist's square root, and whether the pair is aligned"""
    if len(a) * len(b) > pyward.MAX_OPS:
        return abs(len(a) - len(b)), False
    return table[(a, b)], True


class Case:
    def __init__(self, name, segs, seed):
        self.name, self.segs, self.seed, self.n = name, list(segs), seed, len(segs)
        self.order = sorted(range(self.n), key=lambda i: len(self.segs[i]))  # sorted() is stable, as get_spanning_reads' sort is
        self.sorted_segs = [self.segs[i] for i in self.order]
        s = self.sorted_segs
        table = edit_pairs([(s[i], s[j]) for i in range(self.n) for j in range(i + 1, self.n) if len(s[i]) * len(s[j]) <= pyward.MAX_OPS])
        both = [score(s[i], s[j], table) for i in range(self.n) for j in range(i + 1, self.n)]
        self.scores = [k for k, _ in both]  # condensed, in matrix order
        self.n_aligned = sum(1 for _, al in both if al)
        self.equal_lengths = len(set(len(x) for x in s)) == 1

    def dists(self):
        return [math.sqrt(float(k)) for k in self.scores]

    def __repr__(self):
        return "Case(%s, n=%d)" % (self.name, self.n)


def locus(case):
    """the locus that realises the case: what trgt_amd.locus.pack takes"""
    rng = np.random.default_rng([case.seed, 7919])
    lf, rf = rand_dna(rng, 250), rand_dna(rng, 250)
    reads = [rand_dna(rng, int(rng.integers(250, 300))) + lf + seg + rf + rand_dna(rng, int(rng.integers(250, 300))) for seg in case.segs]
    return dict(left_flank=lf, right_flank=rf, motifs=[b"CAG"], genotyper="cluster", tr=TR, reads=reads)


MAX_DEPTH = 10000  # Params(max_depth=...) of every run: no locus here is downsampled
_REFS = {}


def oracle_ref(oracle, case):
    """oracle.locus_analyze of the case's locus: computed once per process"""
    if case.name not in _REFS:
        L = locus(case)
        _REFS[case.name] = oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], genotyper=1, max_depth=MAX_DEPTH)
    return _REFS[case.name]


# ------------------------------------------------------------------------------------------------------------------ the restated answer
Answer = namedtuple("Answer", "groups group1 group2 alleles redo classification n_ed counters")


def vote(segs, group):
    """the consensus of equally long segments that differ by substitutions: every member aligns to the backbone column by column"""
    seqs = [segs[i].decode() for i in group]
    return pyconsensus.repair_consensus(seqs[0], seqs, [[(len(seqs[0]), "M")]] * len(seqs)).encode()


def allele_of(case, group, ref=None):
    """vote() where the group's segments are equally long.  Otherwise the consensus needs an aligner and is taken from ref, a result of the
    oracle for this locus: the allele whose interval (ALLR: the shortest and the longest member) is the group's.  Such an allele is the
    oracle's own.  Only the larger group of either max_ops_edge case has one (reads of 100 and 101, of 125 and 126 bases): for that allele
    the restatement checks the groups, the classification, the kept reads and the number of alignments, not the sequence.  (The reads
    of negative_cutoff-5 differ in length too, but every group there is one read.)"""
    lens = [len(case.sorted_segs[i]) for i in group]
    if min(lens) == max(lens):
        return vote(case.sorted_segs, group)
    assert ref is not None, "a group of unequal lengths needs the alleles from outside"
    hits = [a for a, ci in zip(ref["alleles"], ref["gt_ci"]) if (int(ci[0]), int(ci[1])) == (min(lens), max(lens))]
    assert len(hits) == 1, (case, ref["ALLR"])
    return hits[0].encode()


def answer(case, rules=(), ref=None):
    """genotype_cluster::genotype (:58-152) of the case's segments, ploidy 2, under the given reading of the linkage's rules (items of a
    dict of pyward's parameters).  ref: see allele_of."""
    n, segs = case.n, case.sorted_segs
    c = pyward.Counters()
    mat = case.dists()
    groups = pyward.cluster(mat, n, counters=c, **dict(rules))
    g1, g2 = pyward.genotype_groups(groups)
    allele = lambda g: allele_of(case, g, ref)
    a1, a2 = allele(g1), allele(g2)
    redo_lens = dropped = None
    n_ed = case.n_aligned
    if pyward.small_group_is_outlier(len(a1), len(a2), len(g1), len(g2)):
        e1, e2 = allele(list(range(0, n, 2))), allele(list(range(1, n, 2)))
        redo_lens = (len(e1), len(e2))
        alleles = (e2, e1) if len(e1) > len(e2) else (e1, e2)
    else:
        out = [i for i in range(n) if i not in set(g1) | set(g2)]
        table = edit_pairs([(segs[i], a) for i in out for a in (a1, a2) if len(segs[i]) * len(a) <= pyward.MAX_OPS])
        dropped = {}
        for i in out:
            (k1, al1), (k2, al2) = score(segs[i], a1, table), score(segs[i], a2, table)
            dropped[i] = (math.sqrt(float(k1)), math.sqrt(float(k2)))
            n_ed += al1 + al2
        alleles = (a2, a1) if len(a1) > len(a2) else (a1, a2)
    cls, redo = pyward.classify(n, g1, g2, len(a1), len(a2), dropped, redo_lens, counters=c)
    return Answer(groups, g1, g2, alleles, redo, cls, n_ed, c)


@functools.lru_cache(maxsize=None)
def default_answer(case):
    return answer(case)


# ------------------------------------------------------------------------------------------------------------------ designs
def _grid(rng, L, m):
    """m sites at least 3 bases apart and at least 3 bases from either end"""
    cells = list(range(3, L - 3, 3))
    assert m <= len(cells), (L, m)
    return sorted(int(v) for v in rng.choice(cells, size=m, replace=False))


def _alt(backbone, site, which=0):
    return ALT[backbone[site]][which]


def _put(backbone, subs):
    """subs: {site: which alternative base}"""
    b = bytearray(backbone)
    for s, w in subs.items():
        b[s] = _alt(backbone, s, w)
    return bytes(b)


def _backbone(rng, lo=36, hi=60):
    return rand_dna(rng, int(rng.integers(lo, hi + 1)))


def hypercube(rng, n):
    """reads are subsets of m sites: distances are symmetric differences"""
    bb = _backbone(rng)
    st = _grid(rng, len(bb), int(rng.integers(3, 7)))
    return [_put(bb, {s: 0 for s in st if rng.random() < 0.5}) for _ in range(n)]


def _centres(rng, n, shares):
    bb = _backbone(rng, 54, 60)
    st = _grid(rng, len(bb), 16)
    rng.shuffle(st)
    own, noise = 4, st[4 * (len(shares) - 1):]
    centres = [{s: 0 for s in st[own * (c - 1):own * c]} if c else {} for c in range(len(shares))]
    cuts = np.cumsum([0] + list(shares)) / float(sum(shares))
    segs = []
    for i in range(n):
        c = int(np.searchsorted(cuts, (i + 0.5) / n, side="right")) - 1
        subs = dict(centres[c])
        for s in rng.choice(noise, size=int(rng.integers(0, 5)), replace=False):
            subs[int(s)] = int(rng.integers(0, 3))
        segs.append(_put(bb, subs))
    return [segs[i] for i in rng.permutation(n)]


def two_centres(rng, n):
    """0 to 4 substitutions around either of two centres 4 sites apart, about 70 % / 30 % of the reads"""
    return _centres(rng, n, (7, 3))


def three_centres(rng, n):
    return _centres(rng, n, (6, 3, 1))


def identical_pairs(rng, n):
    """k copies each of a few sequences: merges of dissimilarity 0"""
    bb = _backbone(rng)
    st = _grid(rng, len(bb), 6)
    kinds = [_put(bb, {s: 0 for s in st if rng.random() < 0.5}) for _ in range(max(2, min(6, n // 2)))]
    segs = [kinds[i % len(kinds)] for i in range(n)]
    return [segs[i] for i in rng.permutation(n)]


def chain(rng, n):
    """read i differs from read i + 1 at one site: long nearest-neighbour chains"""
    bb = _backbone(rng, 54, 60)
    st = _grid(rng, len(bb), 16)
    subs, segs = {}, []
    for i in range(n):
        segs.append(_put(bb, subs))
        s = st[i % len(st)]
        if s in subs:
            del subs[s]
        else:
            subs[s] = 0
    return segs


def random_hamming(rng, n):
    """every site of 6 to 12 substituted with a probability of its own, by any of the three other bases"""
    bb = _backbone(rng)
    st = _grid(rng, len(bb), int(rng.integers(6, min(12, (len(bb) - 6) // 3) + 1)))
    p = rng.uniform(0.05, 0.5, size=len(st))
    return [_put(bb, {s: int(rng.integers(0, 3)) for s, q in zip(st, p) if rng.random() < q}) for _ in range(n)]


DESIGNS = dict(hypercube=hypercube, two_centres=two_centres, three_centres=three_centres, identical_pairs=identical_pairs, chain=chain,
               random_hamming=random_hamming)
DESIGN_SIZES = {design: SIZES for design in DESIGNS}  # every design at every size: 78 loci


def make(design, n, seed):
    return Case("%s-%d-%d" % (design, n, seed), DESIGNS[design](np.random.default_rng([seed, n]), n), seed)


@functools.lru_cache(maxsize=None)
def design_list(design):
    return tuple(make(design, n, 1000 + SIZES.index(n)) for n in DESIGN_SIZES[design])


# ------------------------------------------------------------------------------------------------------------------ beyond equal lengths
def _copies(rng, L, spec):
    """spec: [(count, {site index: alternative})]: copies of variants of one backbone of L bases"""
    bb = rand_dna(rng, L)
    st = _grid(rng, L, 1 + max([k for _, subs in spec for k in subs], default=0))
    out = []
    for count, subs in spec:
        out += [_put(bb, {st[k]: w for k, w in subs.items()})] * count
    return out


@functools.lru_cache(maxsize=None)
def special_list(name):
    rng = np.random.default_rng(SPECIAL.index(name) + 500)
    mk = lambda tag, segs: Case("%s-%s" % (name, tag), segs, 500 + SPECIAL.index(name))
    if name == "pair":  # cluster()'s n == 2 case
        return (mk("2", _copies(rng, 40, [(1, {}), (1, {0: 0, 1: 0})])),)
    if name == "max_ops_edge":
        # |a| * |b|: 100 * 100 and 80 * 125 are aligned, 100 * 101 and 80 * 126 are not (> MAX_OPS, not >=); the sort by length permutes
        a = _copies(rng, 100, [(5, {}), (4, {0: 0, 1: 0, 2: 0, 3: 0, 4: 0})])
        b = _copies(rng, 101, [(7, {})])
        one = [x for t in zip(b, a) for x in t] + a[len(b):]
        c = _copies(rng, 80, [(6, {}), (3, {0: 0})])
        d, e = _copies(rng, 125, [(6, {})]), _copies(rng, 126, [(7, {})])
        two = [x for t in zip(e, d, c) for x in t] + c[6:] + e[6:]
        return (mk("100-101", one), mk("80-125-126", two))
    if name == "min_cluster_rounding":
        # 0.01 n = 1.5, 2.5, 3.5 round half away from zero to 2, 3, 4: n - s copies of one sequence and a second cluster of s copies of
        # another, one read short of that (no step qualifies: cluster() splits even / odd, the LATER group, the odd reads, is popped first
        # and becomes class 0) and exactly that (two groups, small_group_is_outlier, the redo: the even reads are class 0)
        out = []
        for n in (150, 250, 350):
            need = max(2, pyward.round_half_away(0.01 * n))
            for s in (need - 1, need):
                segs = _copies(rng, 48, [(n - s, {}), (s, {0: 0, 1: 0, 2: 0, 3: 0, 4: 1, 6: 0, 7: 0, 8: 0})])
                out.append(mk("%d-%d" % (n, s), [segs[i] for i in rng.permutation(n)]))
        return tuple(out)
    if name == "outlier_redo":
        # small_group_is_outlier: min * 4 < max -- 5 * 4 < 20 is false, 5 * 4 < 21 is true; equal allele lengths
        out = []
        for big in (20, 21):
            segs = _copies(rng, 45, [(big, {}), (5, {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0})])
            out.append(mk("%d-5" % big, [segs[i] for i in rng.permutation(big + 5)]))
        return tuple(out)
    if name == "dropped_reads":
        # a lone third read 11 sites away from two groups that are 2 sites apart, so that it merges last: as far from either allele (another
        # base at the sites the alleles differ at), or nearer to the second (its bases there)
        far = {k: 0 for k in range(2, 13)}
        out = []
        for tag, third in (("tie", {**far, 0: 1, 1: 1}), ("nearer", {**far, 0: 0, 1: 0})):
            segs = _copies(rng, 57, [(7, {}), (5, {0: 0, 1: 0}), (1, third)])
            out.append(mk(tag, [segs[i] for i in rng.permutation(13)]))
        return tuple(out)
    if name == "negative_cutoff":
        # A qualifying step of dissimilarity 0 needs two clusters of two reads at distance 0.  Copies of one sequence never give it: with ties
        # to the first index a merged pair, which lives at its larger index, is met before any later copy and absorbs the copies one by one.
        # Four reads of 125 bases are at distance 0 from each other whatever they hold (125 * 125 > MAX_OPS, equal lengths), while a read x of
        # 80 bases is aligned to each (80 * 125 = MAX_OPS) and is nearest to the LAST of them: the chain x -> a4 -> a1 merges (a1, a4) at the
        # largest index, x then finds a2, and a2 finds a3 before that pair.  (a1, a4) + (a2, a3) is the only merge of two clusters of two
        # reads, at 0: the cut-off is -0.0001, no step lies under it and every read is its own group.
        x, tail = _copies(rng, 80, [(1, {}), (1, {0: 0, 1: 0}), (1, {2: 0}), (1, {3: 0, 4: 0, 5: 0})]), rand_dna(rng, 45)
        return (mk("5", [x[1] + tail, x[0], x[2] + tail, x[3] + tail, x[0] + tail]),)
    raise KeyError(name)


SPECIAL = ("pair", "max_ops_edge", "min_cluster_rounding", "outlier_redo", "dropped_reads", "negative_cutoff")


def all_lists():
    """{list name: cases}"""
    out = {d: design_list(d) for d in DESIGNS}
    out.update({s: special_list(s) for s in SPECIAL})
    return out


# ------------------------------------------------------------------------------------------------------------------ the seeded search
@functools.lru_cache(maxsize=None)
def _candidate(size_class, seed):
    lo, hi = SIZE_CLASSES[size_class]
    rng = np.random.default_rng([seed, 31])
    lo = max(lo, 8)
    n = int(rng.integers(lo, min(hi, lo + 40) + 1))
    design = ("random_hamming", "hypercube", "two_centres", "chain")[seed % 4]
    return Case("sensitive-%s-%s-%d" % (size_class, design, seed), DESIGNS[design](rng, n), seed)


def search(rule, size_class, seeds):
    """the seeds whose locus changes its classification under the altered rule -- how SENSITIVE_SEEDS was found"""
    found = []
    for seed in seeds:
        case = _candidate(size_class, seed)
        if answer(case, tuple(RULES[rule].items())).classification != default_answer(case).classification:
            found.append(seed)
    return found


# The first entries of search(rule, size_class, range(0, 400 / 200 / 40)) for the three size classes, which found the classification changed
# on 117 / 94 / 19 seeds for ties_last, 12 / 19 / 10 for lw_order and 80 / 81 / 21 for no_keep_previous.  A changed classification is the
# narrower of the two ways a final answer can change: a changed backbone alone shows in no result of these loci (see the top of this file)
# and does not count.  The search is not repeated by the tests, which check every entry again.
SENSITIVE_SEEDS = {
    ("ties_last", "lds"): (1, 8, 12, 16, 17, 20), ("lw_order", "lds"): (20, 48, 60, 65, 120, 134), ("no_keep_previous", "lds"): (1, 8, 11, 12, 20, 21),
    ("ties_last", "hbm"): (0, 1, 4, 5, 8, 9), ("lw_order", "hbm"): (9, 21, 32, 36, 52, 56), ("no_keep_previous", "hbm"): (0, 1, 4, 7, 8, 9),
    ("ties_last", "deep"): (0, 1, 4), ("lw_order", "deep"): (0, 11, 15), ("no_keep_previous", "deep"): (0, 1, 4),
}
FLOORS = {"lds": 5, "hbm": 5, "deep": 3}  # loci per altered rule


@functools.lru_cache(maxsize=None)
def sensitive(rule, size_class):
    return tuple(_candidate(size_class, seed) for seed in SENSITIVE_SEEDS.get((rule, size_class), ()))


@functools.lru_cache(maxsize=None)
def altered_answer(case, rule):
    return answer(case, tuple(RULES[rule].items()))
