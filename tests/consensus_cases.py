"""Inputs of the consensus-repair tests (tests/test_consensus_cases.py, tests/test_consensus_vote_gpu.py), as data.

A group is (backbone, [(member, ops)]): ops is the member's run-length CIGAR against the backbone, a list of (len, op) with op one of
"=", "M", "X", "D", "I"; an empty list is a member whose alignment failed.  HAND holds one decision of repair_consensus
(consensus.rs:5-111) per vector, with the consensus it must give stated literally; SHAPES holds the sizes at which the device kernel
(256 threads, four waves, votes in LDS up to 4 000 backbone bases) takes another path; random_groups() derives noisy members from a
backbone position by position.  designed_loci() are the haploid cluster-genotyper loci whose every voting segment the tests choose."""
import random

CODE = {"M": 0, "I": 1, "D": 2, "=": 7, "X": 8}  # cigar_get_CIGAR: "MIDNSHP=X"


def words(ops):
    """the dense `len << 4 | code` words of a CIGAR"""
    return [(n << 4) | CODE[op] for n, op in ops]


def _dna(n, seed):
    """n bases of a fixed pseudo-random sequence (a 31-bit LCG; nothing here depends on a library's generator)"""
    out, s = [], seed * 2654435761 % 2147483648 + 12345
    for _ in range(n):
        s = (s * 1103515245 + 12345) % 2147483648
        out.append("ACGT"[(s >> 16) & 3])
    return "".join(out)


# ---------------------------------------------------------------------------------------------------------------- hand-made vectors
# (name, backbone, [(member, ops)], expected consensus).  Counter order: A, T, C, G, deleted; the LAST maximum wins.
HAND = [
    # A = 1, T = 1: T is the later counter
    ("tie A=T", "A", [("A", [(1, "=")]), ("T", [(1, "X")])], "T"),
    # T = 1, C = 1 -> C; given in the other member order than the counters' (the order of the members must not matter)
    ("tie T=C", "T", [("C", [(1, "X")]), ("T", [(1, "=")])], "C"),
    # C = 1, G = 1 -> G
    ("tie C=G", "GCG", [("GCG", [(3, "=")]), ("GGG", [(1, "="), (1, "X"), (1, "=")])], "GGG"),
    # position 1: G = 1, deleted = 1 -> deleted is the last counter, the base goes
    ("tie G=deleted", "CGC", [("CGC", [(3, "=")]), ("CC", [(1, "="), (1, "D"), (1, "=")])], "CC"),
    # position 1: A = T = C = G = deleted = 1 -> deleted
    ("five-way tie", "CAC", [("CAC", [(3, "=")]), ("CTC", [(1, "="), (1, "X"), (1, "=")]), ("CCC", [(1, "="), (1, "X"), (1, "=")]),
                             ("CGC", [(1, "="), (1, "X"), (1, "=")]), ("CC", [(1, "="), (1, "D"), (1, "=")])], "CC"),
    # every alignment failed: all five counters are 0 at every position, the last of the equal maxima is "deleted" -> nothing is left
    ("nobody votes", "ACG", [("ACG", []), ("ACGT", [])], ""),
    # M (code 0) counts the member's base like = and X do; position 2: T = 2, G = 1
    ("M next to = and X", "ACGT", [("ACTT", [(1, "="), (1, "M"), (1, "X"), (1, "M")]), ("ACTT", [(4, "M")]), ("ACGT", [(2, "M"), (2, "=")])], "ACTT"),
    # an insertion is looked at when MORE than n // 2 members have one, and taken when its count exceeds the members without one
    ("ins 0 of 1", "CC", [("CC", [(2, "=")])], "CC"),
    ("ins 1 of 1", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")])], "CAC"),
    ("ins 1 of 2", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [(2, "=")])], "CC"),       # 1 > 1 is false
    ("ins 2 of 2", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")])] * 2, "CAC"),
    ("ins 1 of 3", "CC", [("CC", [(2, "=")]), ("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [(2, "=")])], "CC"),  # 1 > 1 is false
    ("ins 2 of 3", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [(2, "=")]), ("CAC", [(1, "="), (1, "I"), (1, "=")])], "CAC"),  # 2 > 1, count 2 > 1 without
    ("ins 2 of 4", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")])] * 2 + [("CC", [(2, "=")])] * 2, "CC"),  # 2 > 2 is false
    ("ins 3 of 4", "CC", [("CC", [(2, "=")])] + [("CAC", [(1, "="), (1, "I"), (1, "=")])] * 3, "CAC"),     # 3 > 2, count 3 > 1 without
    ("ins 2 of 5", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")])] * 2 + [("CC", [(2, "=")])] * 3, "CC"),  # 2 > 2 is false
    ("ins 3 of 5", "CC", [("CC", [(2, "=")])] * 2 + [("CAC", [(1, "="), (1, "I"), (1, "=")])] * 3, "CAC"),  # 3 > 2, count 3 > 2 without
    # three of five insert (3 > 2), "A" twice: as many as the two members without an insertion -> not taken
    ("count == without", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [(2, "=")]), ("CGC", [(1, "="), (1, "I"), (1, "=")]),
                                 ("CC", [(2, "=")]), ("CAC", [(1, "="), (1, "I"), (1, "=")])], "CC"),
    # five of seven insert, "A" three times against two members without -> taken
    ("count == without + 1", "CC", [("CGC", [(1, "="), (1, "I"), (1, "=")]), ("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [(2, "=")]),
                                     ("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CTC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [(2, "=")]),
                                     ("CAC", [(1, "="), (1, "I"), (1, "=")])], "CAC"),
    # "AC" twice and "ACA" twice: the first of the sorted strings among equals, and a prefix sorts in front of its extension
    ("equal counts, prefix", "CC", [("CACAC", [(1, "="), (3, "I"), (1, "=")]), ("CACC", [(1, "="), (2, "I"), (1, "=")]),
                                     ("CACAC", [(1, "="), (3, "I"), (1, "=")]), ("CACC", [(1, "="), (2, "I"), (1, "=")])], "CACC"),
    # "T" once and "AAA" once: strings are ordered by their bytes first and their lengths last, "AAA" < "T"
    ("equal counts, bytes before length", "CC", [("CTC", [(1, "="), (1, "I"), (1, "=")]), ("CAAAC", [(1, "="), (3, "I"), (1, "=")])], "CAAAC"),
    # an insertion at y = 0 is emitted in front of the first base
    ("ins in front of position 0", "CC", [("GCC", [(1, "I"), (2, "=")])], "GCC"),
    # an insertion at y = len(backbone) is collected and never emitted
    ("ins behind the last position", "CC", [("CCG", [(2, "="), (1, "I")]), ("CCGG", [(2, "="), (2, "I")])], "CC"),
    # position 1: deleted = 2, G = 1 -> the base goes, the insertion in front of it (2 > 1, count 2 > 1 without) stays
    ("ins in front of a deleted position", "CGC", [("CAC", [(1, "="), (1, "I"), (1, "D"), (1, "=")]), ("CGC", [(3, "=")]),
                                                   ("CAC", [(1, "="), (1, "I"), (1, "D"), (1, "=")])], "CAC"),
    # the only member deletes the only base
    ("empty consensus", "A", [("", [(1, "D")])], ""),
    # I then D: the insertion belongs to position 1, whose base (and the next) is deleted
    ("I followed by D", "CGTC", [("CAC", [(1, "="), (1, "I"), (2, "D"), (1, "=")])], "CAC"),
    # D then I: the insertion belongs to position 3, behind the two deleted bases; x advances over it before the last match
    ("D followed by I", "CGTC", [("CTG", [(1, "="), (2, "D"), (1, "I"), (1, "X")])], "CTG"),
    # failed members count in n: 2 insertions of 4 members are not more than half (of the 2 aligned members they would be)
    ("failed members count in n", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")]), ("GGGG", []), ("CAC", [(1, "="), (1, "I"), (1, "=")]), ("CC", [])], "CC"),
    # ... and in "without": 2 of 3 insert (2 > 1), count 2 > 1 failed member without
    ("a failed member has no insertion", "CC", [("CAC", [(1, "="), (1, "I"), (1, "=")]), ("TTT", []), ("CAC", [(1, "="), (1, "I"), (1, "=")])], "CAC"),
    ("backbone of length 1", "G", [("TG", [(1, "I"), (1, "=")])], "TG"),
    ("backbone of length 1, 1 of 2 insert", "G", [("G", [(1, "=")]), ("TG", [(1, "I"), (1, "=")])], "G"),
]

# ---------------------------------------------------------------------------------------------------------------- shape vectors
# (name, backbone, members, expected consensus)


def _ends(L):
    """two of three members insert "TT" in front of the first base and "GA" in front of the last one, and delete the middle base"""
    bb, h = _dna(L, L), L // 2
    if L < 4:
        raise ValueError(L)
    m = "TT" + bb[:h] + bb[h + 1:L - 1] + "GA" + bb[L - 1]
    ops = [(2, "I"), (h, "="), (1, "D"), (L - 2 - h, "="), (2, "I"), (1, "=")]
    return ("ends of %d" % L, bb, [(m, ops), (bb, [(L, "=")]), (m, ops)], m)


def _ballots():
    """candidates at the first and last lanes of the four waves of a 256-position block, and in the next block: each with its own string"""
    pos = [0, 63, 64, 127, 128, 255, 256, 257]
    ins = ["A", "CC", "GTG", "T", "AC", "G", "TTA", "CA"]
    bb = _dna(300, 7)
    m, ops, at = "", [], 0
    for p, s in zip(pos, ins):
        if p > at:
            m += bb[at:p]
            ops.append((p - at, "="))
        m += s
        ops.append((len(s), "I"))
        at = p
    m += bb[at:]
    ops.append((300 - at, "="))
    return ("candidates at the wave ballots' ends", bb, [(bb, [(300, "=")]), (m, ops), (m, ops)], m)


def _same_wave():
    bb = _dna(20, 9)
    m = bb[:10] + "AG" + bb[10] + "T" + bb[11:]
    ops = [(10, "="), (2, "I"), (1, "="), (1, "I"), (9, "=")]
    return ("two candidates in one wave", bb, [(m, ops), (m, ops), (bb, [(20, "=")])], m)


def _code(v):
    """six bases, ordered as v is (A < C < G < T)"""
    return "".join("ACGT"[(v >> (2 * k)) & 3] for k in range(5, -1, -1))


def _members(n):
    """every member inserts a string of its own at position 5, the smallest of them carried by the LAST member: all counts are 1, none is
    without, and the first of the sorted strings wins.  From 257 members on a second candidate at position 20, won by member 256."""
    bb = _dna(33 if n % 2 else 40, n)
    two = n > 256
    members = []
    for j in range(n):
        s1 = _code(n - 1 - j)
        if two:
            s2 = _code((j - 256) % n)
            members.append((bb[:5] + s1 + bb[5:20] + s2 + bb[20:], [(5, "="), (6, "I"), (15, "="), (6, "I"), (len(bb) - 20, "=")]))
        else:
            members.append((bb[:5] + s1 + bb[5:], [(5, "="), (6, "I"), (len(bb) - 5, "=")]))
    exp = bb[:5] + "AAAAAA" + (bb[5:20] + "AAAAAA" + bb[20:] if two else bb[5:])
    return ("%d members" % n, bb, members, exp)


def _long_runs():
    """a run of 65 "=" and one of 130 "D" (more than the 64 lanes that share a run), carried by two of three members"""
    bb = _dna(200, 11)
    m = bb[:65] + bb[195:]
    ops = [(65, "="), (130, "D"), (5, "=")]
    return ("runs of 65 = and 130 D", bb, [(m, ops), (bb, [(200, "=")]), (m, ops)], m)


MEMBER_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 2048)
SHAPES = ([_ends(L) for L in (255, 256, 257, 511, 513, 4000, 4001)] + [_ballots(), _same_wave()] + [_members(n) for n in MEMBER_COUNTS] +
          [_long_runs()])

# ---------------------------------------------------------------------------------------------------------------- seeded random lists
RANDOM_SEEDS = (11, 12, 13)


class _Rng:
    """integers and choices from random.Random(seed).random() alone (the one method whose stream Python guarantees)"""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def u(self):
        return self.r.random()

    def below(self, n):
        return int(self.r.random() * n)

    def pick(self, xs):
        return xs[self.below(len(xs))]

    def subset(self, n, k):
        idx = list(range(n))
        for i in range(k):
            j = i + self.below(n - i)
            idx[i], idx[j] = idx[j], idx[i]
        return set(idx[:k])


def _variants(rng, backbone, n, noise=0.02, thirds=False):
    """n members derived from the backbone position by position.  About one position in six (the one behind the last base included) is
    hot: a fraction 0.3 / 0.5 / 0.7 of the members carries an insertion drawn from one to three short strings, deletes the base or
    substitutes one fixed base there; everywhere else 2 % of the (member, position) pairs do one of the three at random.  Returns
    [(member, ops)] in run-length form (no two adjacent runs of one op).  thirds: the members of a hot position are two of the three classes
    m % 3 instead (a locus of many independent variants has a read that carries every majority feature, which is then the central read
    and leaves the vote nothing to repair)."""
    L = len(backbone)
    plan = []  # per position 0 .. L: None or (kind, chosen members, strings / base)
    for y in range(L + 1):
        if rng.u() >= 1.0 / 6.0:
            plan.append(None)
            continue
        kind = "I" if y == L else rng.pick("IDX")
        k = min(n, max(1, int(rng.pick((0.3, 0.5, 0.7)) * n + 0.5)))
        chosen = rng.subset(n, k)
        if thirds:  # two of the three classes m % 3: no member carries every majority feature, so no backbone is the consensus already
            skip = rng.below(3)
            chosen = set(m for m in range(n) if m % 3 != skip)
        if kind == "I":
            what = ["".join(rng.pick("ACGT") for _ in range(1 + rng.below(3))) for _ in range(1 + rng.below(3))]
        elif kind == "X":
            what = rng.pick([b for b in "ACGT" if b != backbone[y]])
        else:
            what = None
        plan.append((kind, chosen, what))
    out = []
    for m in range(n):
        seq, ops = [], []

        def push(k, op):
            if ops and ops[-1][1] == op:
                ops[-1] = (ops[-1][0] + k, op)
            else:
                ops.append((k, op))
        for y in range(L + 1):
            ins, base = None, "="
            hot = plan[y]
            if hot is not None and m in hot[1]:
                if hot[0] == "I":
                    ins = rng.pick(hot[2])
                elif hot[0] == "D":
                    base = "D"
                else:
                    base = hot[2]
            elif hot is None and rng.u() < noise:
                kind = rng.pick("IDX")
                if kind == "I":
                    ins = rng.pick("ACGT")
                elif kind == "D":
                    base = "D"
                else:
                    base = rng.pick("ACGT")
            if ins is not None:
                seq.append(ins)
                push(len(ins), "I")
            if y == L:
                break
            if base == "D":
                push(1, "D")
            elif base == "=" or base == backbone[y]:
                seq.append(backbone[y])
                push(1, "=")
            else:
                seq.append(base)
                push(1, "X")
        out.append(("".join(seq), ops))
    return out


def random_groups(seed, count=300):
    """[(backbone, [(member, ops)])]: backbones of 1 to 80 bases, 1 to 12 members"""
    rng = _Rng(seed)
    groups = []
    for _ in range(count):
        L, n = 1 + rng.below(80), 1 + rng.below(12)
        bb = "".join(rng.pick("ACGT") for _ in range(L))
        groups.append((bb, _variants(rng, bb, n)))
    return groups


# ---------------------------------------------------------------------------------------------------------------- designed loci
def designed_loci():
    """Haploid cluster-genotyper loci (ploidy 1, Genotyper::Cluster: the genotype is ONE make_consensus over all kept reads): reads are
    pad + left flank + segment + right flank + pad with random 250-base flanks, so the exact flank search locates the spans, and the
    segments are variants of a random 40 to 90-base allele built like the hot positions above.  Depths 1, 2, 3, 12, 30 and 300; one
    locus of 120-base segments (len1 * len2 > MAX_OPS: the distances are sqrt(|length difference|)).  That locus and the one of 300 reads
    take their hot positions' members by thirds, so that their central read is not the consensus already.  Returns dicts for
    trgt_amd.locus.pack plus "segments", "depth" and "long"."""
    loci = []
    # (the seed of the deep locus is one of 80 tried for which the restatement takes an insertion and deletes a base of the central read)
    for depth, seg_len, seed in ((1, 41, 1000), (2, 57, 1001), (3, 40, 1002), (12, 77, 1003), (30, 90, 1004), (30, 120, 1005), (300, 64, 1046)):
        rng = _Rng(seed)
        dna = lambda n: "".join(rng.pick("ACGT") for _ in range(n))
        lf, rf, allele = dna(250), dna(250), dna(seg_len)
        segments = [s for s, _ in _variants(rng, allele, depth, noise=0.01 if seg_len == 120 else 0.02, thirds=seg_len in (120, 64))]
        reads = [(dna(250 + rng.below(50)) + lf + s + rf + dna(250 + rng.below(50))).encode() for s in segments]
        loci.append(dict(left_flank=lf.encode(), right_flank=rf.encode(), motifs=[b"CAG", b"CCG"], genotyper="cluster", ploidy=1,
                         tr=allele.encode(), reads=reads, segments=segments, depth=depth, long=seg_len == 120))
    return loci
