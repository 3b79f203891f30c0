"""The lane-parallel sections of the one-wave size genotyper (trgt_amd/csrc/locus_gt.hpp: LDS layout, unique lengths as runs, equal
reads by hash and comparison before the sorted insertion, picks and majority by ballots, classification a lane per read).

Every case runs three ways on one context each -- the default path, TRGT_GT_SERIAL=1 (a context the developer library creates: every
section read by read, as before) and the CPU oracle's restatement of analyze_tr -- and, where the case is about the sequence
histogram, a fourth time under TRGT_GT_WEAK_HASH=1 (the hash is the length alone: distinct sequences of one length collide, the
comparison fails and the locus inserts every read).  The device runs are compared array for array (alleles, allele_len, ci, num_spanning,
classification, read_rank, n_alleles, flipped, gt_size), the oracle by alleles, kept reads and their order, classification, intervals
and spanning counts.  The oracle's results of a case are computed once.  Loci are hand-made with 40-base flanks so that reads stay
small: read = pad + left flank + segment + right flank + pad."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 40
ARRAYS = ("n_alleles", "allele_len", "num_spanning", "classification", "read_rank", "flipped", "gt_size", "span_start", "span_end")


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def ctxs():
    """default, serial, weak hash; the last two also print the tally (TRGT_WFA_DEBUG), as does `tally`, a default context"""
    from trgt_amd import _lib
    c = dict(default=_lib.Context(0), serial=_lib.context_with_env(TRGT_GT_SERIAL=1), weak=_lib.context_with_env(TRGT_GT_WEAK_HASH=1, TRGT_WFA_DEBUG=1),
             tally=_lib.context_with_env(TRGT_WFA_DEBUG=1))
    yield c
    for x in c.values():
        x.close()


class Maker:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.lf, self.rf = self.dna(F), self.dna(F)

    def dna(self, n, alphabet=b"ACGT"):
        return bytes(self.rng.choice(list(alphabet), size=n).tolist())

    def read(self, seg):
        return self.dna(int(self.rng.integers(4, 12))) + self.lf + seg + self.rf + self.dna(int(self.rng.integers(4, 12)))

    def unkept(self, seg):
        """the left flank is cut: located or not, the span starts before flank_len"""
        return self.lf[F // 2:] + seg + self.rf + self.dna(8)

    def locus(self, segs, tr=None, ploidy=2, unkept=()):
        reads = [self.unkept(s) if i in unkept else self.read(s) for i, s in enumerate(segs)]
        return dict(left_flank=self.lf, right_flank=self.rf, tr=tr if tr is not None else (segs[0] if segs else b"CAG"), motifs=[b"CAG", b"A"], ploidy=ploidy,
                    reads=reads, genotyper="size")


def _params(locus, **kw):
    return locus.Params(search_flank_len=F, **kw)


def _oracle(oracle, L, params):
    if L.get("ploidy", 2) == 0:  # Ploidy::Zero is LocusResult::empty (tr.rs:29-31); the oracle's entry point knows ploidy 1 and 2 only
        return dict(n_alleles=0, alleles=[], kept_read=[], classification=[], gt_ci=[], num_spanning=[])
    return oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], flank_len=params.search_flank_len,
                                min_flank_id_frac=params.min_flank_id_frac, max_depth=params.max_depth, scoring=params.aln_scoring,
                                ploidy=L.get("ploidy", 2), genotyper=0, min_read_qual=params.min_read_qual)


def _same(locus, b, one, other, how):
    for name in ARRAYS:
        assert np.array_equal(getattr(one, name), getattr(other, name)), (how, name)
    # (no kernel writes the interval of an allele the locus does not have: ci is compared where n_alleles says it is defined)
    defined = np.repeat(np.arange(2)[None, :] < one.n_alleles[:, None], 2, axis=1).reshape(-1)
    assert np.array_equal(one.ci[defined], other.ci[defined]), (how, "ci")
    for l in range(int(b["n_loci"])):
        assert locus.locus_result(b, one, l) == locus.locus_result(b, other, l), (how, l)


def _against_oracle(locus, b, out, refs, how):
    for l, ref in enumerate(refs):
        got = locus.locus_result(b, out, l)
        assert [a.seq.decode() for a in got.genotype] == ref["alleles"], (how, l)
        assert got.reads == [int(v) for v in ref["kept_read"]], (how, l)
        assert got.classification == [int(v) for v in ref["classification"]], (how, l)
        assert [a.ci for a in got.genotype] == [tuple(int(v) for v in c) for c in ref["gt_ci"]], (how, l)
        assert [a.num_spanning for a in got.genotype] == [int(v) for v in ref["num_spanning"]], (how, l)


def _tally(err):
    m = re.findall(r"\[size gt\] of (\d+) loci: unsorted (\d+), not staged (\d+), hash collision (\d+)", err)
    assert m, err
    return tuple(int(v) for v in m[-1])


def _three_ways(oracle, locus, ctxs, loci, params, weak=False, capfd=None):
    """-> (batch, oracle results, tally of the default path[, tally under the weak hash])"""
    b = locus.pack(loci)
    refs = [_oracle(oracle, L, params) for L in loci]
    out = locus.run_batch(b, params, ctx=ctxs["default"])
    _against_oracle(locus, b, out, refs, "default")
    _same(locus, b, out, locus.run_batch(b, params, ctx=ctxs["serial"]), "serial")
    tallies = []
    if capfd is not None:
        capfd.readouterr()
        _same(locus, b, out, locus.run_batch(b, params, ctx=ctxs["tally"]), "tally")
        tallies.append(_tally(capfd.readouterr().err))
        if weak:
            _same(locus, b, out, locus.run_batch(b, params, ctx=ctxs["weak"]), "weak hash")
            tallies.append(_tally(capfd.readouterr().err))
    return (b, refs) + tuple(tallies)


X, Y = b"CAGCAGCAGCAGCAGCAGCAG", b"CAGCAGCAGCAGCAGCAGCAGCAGCAGCAG"  # 21 and 30 bases


def test_compaction_and_widths(oracle, locus, ctxs):
    """unkept reads first, in the middle and last; 1, 2, 63, 64 reads (<64>); no kept read; ploidy 0, 1, 2"""
    mk = Maker(1)
    het = lambda n: [X if i % 2 else Y for i in range(n)]
    loci = [mk.locus(het(12), unkept=(0, 1)), mk.locus(het(12), unkept=(5, 6)), mk.locus(het(12), unkept=(10, 11)), mk.locus(het(9), unkept=(0, 4, 8)),
            mk.locus(het(1)), mk.locus(het(2)), mk.locus(het(63)), mk.locus(het(64)), mk.locus(het(3), unkept=(0, 1, 2)),
            mk.locus(het(10), ploidy=0), mk.locus(het(10), ploidy=1), mk.locus([X] * 7 + [Y], ploidy=1), mk.locus(het(10), ploidy=2)]
    b, refs = _three_ways(oracle, locus, ctxs, loci, _params(locus))
    assert [len(r["kept_read"]) for r in refs[:9]] == [10, 10, 10, 6, 1, 2, 63, 64, 0]


def test_widths_of_the_large_form(oracle, locus, ctxs):
    """65, 128 and 256 reads (GT_BIG); runs of equal lengths that cross the 64-element boundaries; ties on both sides of element 64"""
    mk = Maker(2)
    seg = lambda n: (b"CA" * 40)[:n]
    runs = [seg(10)] * 60 + [seg(11)] * 10 + [seg(12)] * 70 + [seg(13)] * 50  # boundaries at 60, 70, 140: runs cross 64 and 128
    ties = [seg(20)] * 60 + [seg(24)] * 60 + [seg(22)] * 10                  # 22 is tied between 20 and 24: ranks 60 .. 69, across element 64
    order = mk.rng.permutation(len(runs))
    loci = [mk.locus([X if i % 2 else Y for i in range(65)]), mk.locus([X if i % 3 else Y for i in range(128)]), mk.locus([X if i % 2 else Y for i in range(256)]),
            mk.locus([runs[i] for i in order]), mk.locus(ties), mk.locus([seg(30)] * 130)]
    b, refs = _three_ways(oracle, locus, ctxs, loci, _params(locus, max_depth=10000))
    assert [len(r["kept_read"]) for r in refs] == [65, 128, 256, 190, 130, 130]
    assert sorted(set(len(a) for a in refs[4]["alleles"])) == [20, 24]
    cls = refs[5]["classification"].tolist()  # one length, two equal alleles: every read ties, the toggle runs through all 130
    assert all(cls[i] == i % 2 for i in range(130))


def test_unique_lengths(oracle, locus, ctxs, capfd):
    """all equal, all different, and max_depth below n (8 of 20 or 30 reads).  The downsample swaps position i with position floor(i * step),
    step > 1: the positions it reads from rise strictly and lie at or behind i, so the kept prefix is still sorted by length and the
    tally counts no unsorted list"""
    mk = Maker(3)
    seg = lambda n: (b"CAG" * 30)[:n]
    loci = [mk.locus([seg(25)] * 20), mk.locus([seg(10 + i) for i in mk.rng.permutation(30)]), mk.locus([seg(12 + (i * 7) % 20) for i in range(20)])]
    b, refs, tally = _three_ways(oracle, locus, ctxs, loci, _params(locus), capfd=capfd)
    assert tally == (3, 0, 0, 0)
    b, refs, tally = _three_ways(oracle, locus, ctxs, loci, _params(locus, max_depth=8), capfd=capfd)
    assert [len(r["kept_read"]) for r in refs] == [8, 8, 8]
    assert tally == (3, 0, 0, 0)


def _histogram_loci(mk):
    s = bytearray(b"CAGT" * 6)  # 24 bases

    def flip(at):
        t = bytearray(s)
        t[at] = ord("A") if t[at] != ord("A") else ord("C")
        return bytes(t)
    base = bytes(s)
    tails = [mk.locus([(b"CAGCAGC")[:n]] * 3 + [(b"CAGCAGC")[:n - 1] + b"T"] * 2) for n in (1, 2, 3, 5, 6, 7)]  # lengths 1, 3, 5 and 1, 2, 3 mod 4
    return tails + [
        mk.locus([base] * 9),                                           # all reads identical
        mk.locus([base, flip(0)] * 4 + [base]),                         # ... differing only in the first byte
        mk.locus([base, flip(23)] * 4 + [base]),                        # ... only in the last byte
        mk.locus([base, flip(3)] * 4 + [base]),                         # ... only at byte 3
        mk.locus([base, flip(4)] * 4 + [base]),                         # ... only at byte 4 (dword edge)
        mk.locus([base[:12]] * 4 + [base] * 5),                         # one sequence a proper prefix of another
        mk.locus([b"TTTTTTTTTTTT"] * 2 + [b"AAAAAAAAAAAA"] * 2 + [b"CCCCCCCCCCCC"] * 2 + [b"GGGGGGGGGGGG"] * 2),  # the first read the largest
        mk.locus([b"CAGCAGCAGCAG", b"CAGCAGCAGCAT"] * 4),               # equal counts: most_frequent takes the last in byte order
        mk.locus([b"CAGCAGCAGCAT", b"CAGCAGCAGCAG"] * 4),               # ... whichever comes first in the reads
        mk.locus([(b"CA" * 20)[:18]] * 5 + [(b"CA" * 20)[:22]] * 5 + [(b"CA" * 20)[:20]] * 10 + [(b"CA" * 20)[:40]] * 10),  # 18 and 22 equidistant from 20
        mk.locus([flip(i % 24) for i in range(24)]),                    # 24 distinct sequences of one length: no majority, the repair chain
    ]


def test_sequence_histogram(oracle, locus, ctxs, capfd):
    mk = Maker(4)
    loci = _histogram_loci(mk)
    b, refs, tally, weak = _three_ways(oracle, locus, ctxs, loci, _params(locus), weak=True, capfd=capfd)
    assert tally == (len(loci), 0, 0, 0)          # no collision without the switch
    assert weak == (len(loci), 0, 0, 14)           # every locus with two sequences of one length collides under it: all but three
    assert refs[-1]["stats"]["n_wfa_cons"] > 0    # (the last locus went through repair_consensus in the oracle)


def test_classification_ties(oracle, locus, ctxs):
    """1, 2 and 3 tied reads between two alleles"""
    mk = Maker(5)
    seg = lambda n: (b"CAG" * 20)[:n]
    loci = [mk.locus([seg(20)] * 8 + [seg(24)] * 8 + [seg(22)] * k) for k in (1, 2, 3)]
    b, refs = _three_ways(oracle, locus, ctxs, loci, _params(locus))
    for k, r in zip((1, 2, 3), refs):
        assert sorted(len(a) for a in r["alleles"]) == [20, 24]
        tied = [int(c) for c, i in zip(r["classification"], r["kept_read"]) if int(r["span_end"][i] - r["span_start"][i]) == 22]
        assert len(tied) == k and all(c in (0, 1) for c in tied)


def test_no_majority(oracle, locus, ctxs):
    """noisy reads: the picks lack majority support, the repair queue's groups and the finished alleles are the oracle's"""
    mk = Maker(6)
    noisy = lambda s: bytes(int(mk.rng.choice(list(b"ACGT"))) if mk.rng.random() < 0.06 else c for c in s)
    loci = [mk.locus([noisy(b"CAG" * 12 if i % 2 else b"CAG" * 17) for i in range(n)], tr=b"CAG" * 12) for n in (20, 40, 90)]
    b, refs = _three_ways(oracle, locus, ctxs, loci, _params(locus, max_depth=10000))
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs)


def test_does_not_fit(oracle, locus, ctxs, capfd):
    """30 reads of about 300 bases in <64, 8 KB>: the segments are compared where they lie, the tally says so"""
    mk = Maker(7)
    a, c = b"CAG" * 100, b"CAG" * 96 + b"CCG" * 5
    loci = [mk.locus([a if i % 2 else c for i in range(30)], tr=a), mk.locus([X] * 5)]
    b, refs, tally = _three_ways(oracle, locus, ctxs, loci, _params(locus), capfd=capfd)
    assert tally == (2, 0, 1, 0)


def test_flank_and_snv_forms(oracle, locus):
    """the FLANK and SNV instantiations: a haplotagged locus and one with mismatch offsets, duplicate sequences in both groups
    (f_uidx, flank_tail); default path and TRGT_GT_SERIAL=1 against the oracle with the read metadata"""
    from trgt_amd import _lib
    import snv_split_cases as sc
    from test_flank_device_gpu import _compare, _expected_stats, _het, _ref
    rng = np.random.default_rng(8)
    params = locus.Params()
    for setter, loci in (("set_flank_device", [_het(rng, 12), _het(rng, 31)]), ("set_snv_split_device", [sc.het(rng, 12), sc.het(rng, 30)])):
        b = locus.pack(loci)
        refs = [_ref(oracle, L, params) for L in loci]
        plain = [_ref(oracle, L, params, meta=False) for L in loci]
        want = _expected_stats(loci, plain) if setter == "set_flank_device" else sc.expected_stats(loci, plain)
        assert want[0] == 2 and want[2:] == (0, 0), want  # both loci are split on the device
        outs = []
        for how, ctx in (("default", _lib.Context(0)), ("serial", _lib.context_with_env(TRGT_GT_SERIAL=1))):
            try:
                getattr(ctx, setter)(True)
                outs.append(locus.run_batch(b, params, ctx=ctx))
                _compare(locus, b, outs[-1], refs, (setter, how))
                stats = ctx.flank_stats() if setter == "set_flank_device" else ctx.snv_split_stats()
                assert stats == want, (setter, how, stats)
            finally:
                ctx.close()
        _same(locus, b, outs[0], outs[1], setter)


@pytest.fixture(scope="module")
def random_loci():
    """300 loci of 1-64 reads and 100 of 65-256: segments over two bases, 1-40 long, drawn so that duplicates, prefixes and ties are common"""
    mk = Maker(20261021)

    def one(n):
        pool = [mk.dna(int(mk.rng.integers(1, 41)), b"CA") for _ in range(int(mk.rng.integers(1, 7)))]
        pool += [p[:max(1, len(p) - int(mk.rng.integers(0, 3)))] for p in pool[:2]]
        return mk.locus([pool[int(mk.rng.integers(0, len(pool)))] for _ in range(n)], tr=pool[0], ploidy=int(mk.rng.choice([1, 2, 2, 2])))
    return [one(int(mk.rng.integers(1, 65))) for _ in range(300)], [one(int(mk.rng.integers(65, 257))) for _ in range(100)]


@pytest.mark.parametrize("big", [False, True])
def test_random_loci(oracle, locus, ctxs, random_loci, big):
    _three_ways(oracle, locus, ctxs, random_loci[big], _params(locus, max_depth=10000 if big else 250))
