"""Hand-made loci for filter_impure_trs (src/trgt/workflows/tr.rs:37-50, 400-452), shared by tests/test_purity_filter_order.py (the
arithmetic, on the CPU) and tests/test_purity_filter_device_gpu.py (the device kernels).  Every locus has 250-base flanks and at most
40 reads, except the one that is there to be oversized.  Read qualities: 0.999 = not scored (purity exactly 1.0), 0.7 and None = scored."""
import numpy as np

CAG20 = b"CAG" * 20


class Maker:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.lf, self.rf = self.dna(250), self.dna(250)

    def dna(self, n):
        return bytes(self.rng.choice(list(b"ACGT"), size=n).tolist())

    def read(self, rep):
        return self.dna(int(self.rng.integers(250, 300))) + self.lf + rep + self.rf + self.dna(int(self.rng.integers(250, 300)))

    def impure(self, rep, k):
        """k substitutions at distinct places: 14 of 60 bases put a CAG repeat well below purity 0.9, up to 2 leave it above"""
        rep = bytearray(rep)
        for i in self.rng.choice(len(rep), size=k, replace=False):
            rep[i] = ord("T") if rep[i] != ord("T") else ord("A")
        return bytes(rep)

    def locus(self, reps, rq, tr=CAG20, motifs=(b"CAG",), **kw):
        assert len(reps) == len(rq)
        return dict(left_flank=self.lf, right_flank=self.rf, tr=tr, motifs=list(motifs), reads=[self.read(r) for r in reps], read_qual=list(rq), **kw)


def budget_loci(seed=101):
    """max_filter = max(1, round(0.1 n)), half away from zero: n = 4 all impure (one dropped), n = 5 / 15 / 25 (round(0.5) = 1,
    round(1.5) = 2, round(2.5) = 3) with more impure reads than that, and ten impure reads of which the budget lets one go"""
    m = Maker(seed)
    out = []
    for n, n_bad in ((4, 4), (5, 3), (15, 5), (25, 6), (10, 10)):
        reps = [m.impure(CAG20, 14) if i < n_bad else m.impure(CAG20, int(m.rng.integers(0, 3))) for i in range(n)]
        order = m.rng.permutation(n)
        out.append(m.locus([reps[i] for i in order], [None if m.rng.random() < 0.5 else 0.7 for _ in range(n)]))
    return out


def ordering_loci(seed=102):
    """equal purity bits at different places of the input order (all segments have one length, so the sort by span length leaves the
    input order alone): only a stable sort by purity reproduces read_rank.  Scored pure reads tie with the unscored ones at 1.0."""
    m = Maker(seed)
    x, y, z = m.impure(CAG20, 14), m.impure(CAG20, 10), m.impure(CAG20, 1)
    reps = [x, CAG20, y, CAG20, z, x, CAG20, y, z, x, CAG20, CAG20]
    rq = [None, 0.999, 0.7, None, 0.7, 0.7, 0.999, None, None, None, 0.7, 0.999]
    loci = [m.locus(reps, rq)]
    # an impure read the filter never sees (quality >= 0.9) in front of the same segment scored
    loci.append(m.locus([x, x, CAG20, y, CAG20, CAG20, x, CAG20], [0.999, None, None, 0.999, 0.7, None, 0.7, 0.999]))
    # every read has rq >= 0.9: no job, the order is untouched although the segments are impure
    loci.append(m.locus([x, CAG20, y, z, CAG20 + b"CAG", x, CAG20], [0.999, 0.95, 0.9, 0.999, 0.91, 0.999, 0.999]))
    return loci


def nan_loci(seed=103):
    """a read whose flanks are adjacent has an empty repeat segment: purity NaN when it is scored, 1.0 when it is not; NaN is not >= 0.9,
    so the walk drops it while the budget lasts"""
    m = Maker(seed)
    c5 = b"CAG" * 5
    bad = m.impure(b"CAG" * 12, 5)
    return [
        m.locus([c5, b"", c5, c5, b"", c5], [None, None, 0.7, 0.999, 0.999, None], tr=c5),          # scored NaN with budget left, unscored empty
        m.locus([c5, b"", bad, c5, c5, c5, bad], [None, 0.7, None, 0.7, 0.999, None, 0.7], tr=c5),  # the budget (1) is gone when the NaN read comes
        m.locus([b"", b"", b""], [None, 0.7, None], tr=b"", motifs=(b"A",)),                       # nothing but NaN
    ]


def envelope_loci(seed=104):
    m = Maker(seed)
    x = m.impure(CAG20, 14)
    return [
        m.locus([CAG20, x, CAG20], [None, None, 0.7], ploidy=0),
        m.locus([CAG20, x, CAG20, b"CAG" * 21, CAG20, x, CAG20], [None, 0.7, 0.7, None, 0.999, None, None], ploidy=1),
        dict(left_flank=m.lf, right_flank=m.rf, tr=CAG20, motifs=[b"CAG"], reads=[m.dna(700) for _ in range(4)], read_qual=[None, 0.7, 0.999, None]),
        m.locus([], []),
    ]


def hmm_class_loci(seed=105):
    """motif sets of the position-per-lane fills (up to 7, 15 and 63 positions: 8, 16, 64 lanes) and of the state-per-lane fill (more)"""
    m = Maker(seed)
    out = []
    vntr = m.dna(60)
    wide = m.dna(70)
    for motifs, units in (((b"CAG",), (20, 26)), ((b"AAAAG", b"AAGGG"), (9, 14)), ((vntr,), (4, 6)), ((wide,), (3, 5)), ((b"CAG", b"CCG", m.dna(60)), (6, 8))):
        def allele(k):
            return b"".join(mo * k for mo in motifs)
        reps = []
        for i in range(10):
            a = allele(units[i % 2])
            reps.append(m.impure(a, len(a) // 4) if i in (1, 6, 7) else m.impure(a, int(m.rng.integers(0, 2))))
        out.append(m.locus(reps, [None, 0.7, 0.999, None, None, 0.7, None, 0.999, 0.7, None], tr=allele(units[0]), motifs=motifs))
    return out


def cluster_loci(seed=106):
    m = Maker(seed)
    noisy = lambda rep: bytes(int(m.rng.choice(list(b"ACGT"))) if m.rng.random() < 0.03 else c for c in rep)
    base = dict(motifs=(b"CAG", b"CCG"), genotyper="cluster")
    reps = [noisy(b"CAG" * 8 + b"CCG" * (3 if i % 2 else 9)) for i in range(20)] + [m.impure(b"CAG" * 8 + b"CCG" * 9, 14), m.impure(b"CAG" * 8 + b"CCG" * 3, 9)]
    order = m.rng.permutation(len(reps))
    return [
        m.locus([reps[i] for i in order], [None if m.rng.random() < 0.6 else (0.7 if m.rng.random() < 0.5 else 0.999) for _ in reps], tr=b"CAG" * 8, **base),
        m.locus([b"CAG" * 9, m.impure(b"CAG" * 9, 7), b"CAG" * 12], [None, None, 0.7], tr=b"CAG" * 8, **base),
    ]


def downsample_loci(seed=107):
    """40 spanning reads, max_depth = 16: get_spanning_reads downsamples BEFORE the filter, so impure reads inside and outside the 16
    are needed to tell the two orders apart (lengths differ, so the sort by span length moves the reads first)"""
    m = Maker(seed)
    reps, rq = [], []
    for i in range(40):
        k = 18 + i % 5
        reps.append(m.impure(b"CAG" * k, 14) if i % 3 == 0 else b"CAG" * k)
        rq.append(None if i % 4 else 0.999)
    loci = [m.locus(reps, rq)]
    loci.append(m.locus(reps[:30], [None] * 30, motifs=(b"CAG", b"CCG"), genotyper="cluster"))
    return loci


def no_majority_loci(seed=108, n_loci=4):
    """length genotyper loci whose pick lacks majority support (every read has its own substitution): consensus repair is needed"""
    m = Maker(seed)
    out = []
    for l in range(n_loci):
        k = 18 + l
        reps = [m.impure(b"CAG" * k, 1) for _ in range(10)] + [m.impure(b"CAG" * k, 14), m.impure(b"CAG" * (k + 9), 1), m.impure(b"CAG" * (k + 9), 2), m.impure(b"CAG" * (k + 9), 1)]
        order = m.rng.permutation(len(reps))
        out.append(m.locus([reps[i] for i in order], [(0.999, 0.7, None)[int(m.rng.integers(0, 3))] for _ in reps], tr=b"CAG" * k))
    return out


def oversized_locus(seed=109):
    """more reads than the device genotyper takes: the host path, which filters the locus itself"""
    m = Maker(seed)
    reps = [m.impure(b"CAG" * (9 if i % 2 else 14), 6) if i % 25 == 0 else b"CAG" * (9 if i % 2 else 14) for i in range(300)]
    reads = [m.dna(3) + m.lf + r + m.rf + m.dna(3) for r in reps]
    return dict(left_flank=m.lf, right_flank=m.rf, tr=b"CAG" * 9, motifs=[b"CAG"], reads=reads, read_qual=[None if i % 3 else 0.7 for i in range(300)])


# ---- the arithmetic of tr.rs:438-448, restated in a few lines (what purity_filter_kernel restates on the device)
def total_cmp_key(x):
    """f64::total_cmp as an integer order on the bits"""
    b = int(np.array([x], np.float64).view(np.int64)[0])
    return b ^ (((b >> 63) & 0xFFFFFFFFFFFFFFFF) >> 1)


def max_filter(n):
    r = 0.1 * float(n)
    return max(1, int(np.floor(r + 0.5)) if r >= 0 else -int(np.floor(-r + 0.5)))  # half away from zero


def filter_order(purities):
    """indices of the reads that stay, in output order: stable sort by total_cmp, then at most max_filter(n) reads below 0.9 go"""
    n = len(purities)
    order = sorted(range(n), key=lambda i: total_cmp_key(purities[i]))  # (sorted() is stable)
    keep, filtered, budget = [], 0, max_filter(n)
    for i in order:
        if purities[i] >= 0.9 or filtered >= budget:
            keep.append(i)
        else:
            filtered += 1
    return keep
