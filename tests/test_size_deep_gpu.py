"""Genotyper::Size loci deeper than 256 reads on the device (locus_gt_deep.hpp, opt-in per context through trgt_hip_set_size_max_reads):
parity with the CPU oracle's restatement of analyze_tr -- spans, alleles, kept reads and their order, classification, AL / ALLR / SD / MC /
MS / AP -- with host reads and with reads resident in HBM, for every branch of genotype_size::genotype at these depths, the planner's
boundaries, the setter and the statistics of trgt_hip_size_deep_stats.

Loci are hand-made like those of test_cluster_deep_gpu.py: 250-base flanks, repeat segments of 24-60 bases unless a case says otherwise.
The oracle's result of a locus is computed once and compared with both runs; no locus of any case is left out of the comparison."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


def _lib_mod():
    from trgt_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def limit():
    return _lib_mod().size_max_reads_limit()


@pytest.fixture(scope="module")
def deep_ctx(limit):
    ctx = _lib_mod().Context(0)
    ctx.set_size_max_reads(limit)
    yield ctx
    ctx.close()


A, B = b"CAG" * 8 + b"CCG" * 3, b"CAG" * 8 + b"CCG" * 9  # 33 and 51 bases


class Maker:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.lf, self.rf = self.dna(250), self.dna(250)

    def dna(self, n):
        return bytes(self.rng.choice(list(b"ACGT"), size=n).tolist())

    def read(self, rep):
        return self.dna(int(self.rng.integers(250, 300))) + self.lf + rep + self.rf + self.dna(int(self.rng.integers(250, 300)))

    def noisy(self, rep, rate=0.03):
        return bytes(int(self.rng.choice(list(b"ACGT"))) if self.rng.random() < rate else c for c in rep)

    def base(self, **kw):
        return dict(dict(left_flank=self.lf, right_flank=self.rf, motifs=[b"CAG", b"CCG"], genotyper="size", tr=A), **kw)

    def het(self, n, rate=0.0, **kw):
        """two alleles, every other read; rate: substitutions per base (0: every read carries an exact allele)"""
        return self.base(reads=[self.read(self.noisy(A if i % 2 else B, rate) if rate else (A if i % 2 else B)) for i in range(n)], **kw)

    def cluster_het(self, n):
        return self.base(genotyper="cluster", tr=b"CAG" * 8, reads=[self.read(self.noisy(b"CAG" * 8 + b"CCG" * (3 if i % 2 else 9))) for i in range(n)])


def _oracle_locus(oracle, b, l, params):
    a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
    reads = [bytes(b["read_blob"][int(b["read_off"][r]):int(b["read_off"][r]) + int(b["read_len"][r])]) for r in range(a0, a1)]
    lf = bytes(b["flank_blob"][int(b["lf_off"][l]):int(b["lf_off"][l]) + int(b["lf_len"][l])])
    rf = bytes(b["flank_blob"][int(b["rf_off"][l]):int(b["rf_off"][l]) + int(b["rf_len"][l])])
    tr = bytes(b["tr_blob"][int(b["tr_off"][l]):int(b["tr_off"][l]) + int(b["tr_len"][l])])
    m0, m1 = int(b["set_motif_begin"][l]), int(b["set_motif_begin"][l + 1])
    motifs = [bytes(b["motif_blob"][int(b["motif_off"][m]):int(b["motif_off"][m + 1])]) for m in range(m0, m1)]
    gt = int(b["genotyper"][l]) if b.get("genotyper") is not None else 0
    rq = b["read_qual"][a0:a1] if b.get("read_qual") is not None else None
    return oracle.locus_analyze(lf, rf, tr, motifs, reads, flank_len=params.search_flank_len,
                                min_flank_id_frac=params.min_flank_id_frac, max_depth=params.max_depth,
                                scoring=params.aln_scoring, ploidy=int(b["ploidy"][l]), genotyper=gt,
                                min_read_qual=params.min_read_qual, read_qual=rq)


def _refs(oracle, b, params):
    return [_oracle_locus(oracle, b, l, params) for l in range(int(b["n_loci"]))]


def _compare(locus, b, out, refs):
    """the fields of test_locus_gpu.py::_compare, against results of the oracle computed once"""
    for l, ref in enumerate(refs):
        a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        assert np.array_equal(out.span_start[a0:a1], ref["span_start"]), l
        assert np.array_equal(out.span_end[a0:a1], ref["span_end"]), l
        got = locus.locus_result(b, out, l)
        assert len(got.genotype) == ref["n_alleles"], l
        assert [a.seq.decode() for a in got.genotype] == ref["alleles"], l
        assert got.reads == [int(v) for v in ref["kept_read"]], l
        assert got.classification == [int(v) for v in ref["classification"]], l
        if ref["n_alleles"]:
            f = got.vcf_fields()
            for k in ("AL", "ALLR", "SD", "MC", "MS", "AP"):
                assert f[k] == ref[k], (l, k)


def _runs(locus, b, params, ctx):
    """host reads, then reads resident in HBM"""
    import torch
    yield "host reads", locus.run_batch(b, params, ctx=ctx)
    reads_dev = torch.from_numpy(b["read_blob"]).cuda()
    flank_dev = torch.from_numpy(b["flank_blob"]).cuda()
    yield "device", locus.run_batch(b, params, ctx=ctx, flank_dev=flank_dev, reads_dev=reads_dev)


def _repaired(b, refs, lo=256, hi=2048):
    """deep size loci (lo < reads <= hi) whose genotype went through repair_consensus in the oracle"""
    n = 0
    for l, ref in enumerate(refs):
        nr = int(b["locus_read_begin"][l + 1]) - int(b["locus_read_begin"][l])
        n += int(b["genotyper"][l]) == 0 and lo < nr <= hi and ref["stats"]["n_wfa_cons"] > 0
    return n


def _check(oracle, locus, loci, params, ctx, stats):
    """stats: what trgt_hip_size_deep_stats must report after either run"""
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    for mode, out in _runs(locus, b, params, ctx):
        _compare(locus, b, out, refs)
        assert ctx.size_deep_stats() == tuple(stats) + (0,), (mode, ctx.size_deep_stats())
    return b, refs


DEEP = dict(max_depth=10000)


def case_many_lengths(mk, mirror):
    """case 8: about 400 reads over 150 distinct lengths (30 .. 179 bases), one sequence per length.  mirror: the histogram is symmetric
    about its middle with two plateaus of two lengths each, so that mirrored candidate pairs have the same penalty terms"""
    lengths = list(range(30, 180))
    seq = {L: mk.noisy((b"CAG" * 60)[:L], 0.05) for L in lengths}
    count = {L: 1 for L in lengths}
    if mirror:
        for L in (70, 71, 138, 139):  # 70 + 139 = 71 + 138 = 30 + 179
            count[L] = 60
    else:
        for L, c in ((62, 80), (63, 25), (131, 100), (133, 35), (40, 5), (170, 9)):
            count[L] = c
    reps = [seq[L] for L in lengths for _ in range(count[L])]
    order = mk.rng.permutation(len(reps))
    return mk.base(tr=seq[70], reads=[mk.read(reps[i]) for i in order])


def diploid_penalties(lens):
    """diploid.rs:5-103 restated: the penalty of every candidate pair of unique lengths, summed in ascending order of the histogram"""
    sizes, counts = np.unique(np.asarray(lens, np.int64), return_counts=True)
    pens = {}
    for si in range(len(sizes)):
        for li in range(si, len(sizes)):
            sa, la = int(sizes[si]), int(sizes[li])
            frac = 0.25 if abs(sa - la) <= 100 else 0.05
            pen = 0.0
            for s, c in zip(sizes.tolist(), counts.tolist()):
                st = 10 + 2 * abs(sa - s) if s != sa else 0
                lt = 10 + 2 * abs(la - s) if s != la else 0
                pen += (float(min(st, lt)) + frac * float(max(st, lt))) * float(c)
            pens[(sa, la)] = pen
    return pens


def case_collapse(mk):
    """case 9: 70 % of 300 reads have 36 bases, the rest lie within +-3 bases"""
    others = [33, 34, 35, 37, 38, 39]
    reps = [b"CAG" * 12] * 210 + [(b"CAG" * 13)[:others[i % 6]] for i in range(90)]
    order = mk.rng.permutation(300)
    return mk.base(tr=b"CAG" * 12, reads=[mk.read(reps[i]) for i in order])


def case_long_reference_first(mk):
    """case 10: alleles of 540 and 600 bases, the reference repeat is the longer one"""
    short, long_ = b"CAG" * 180, b"CAG" * 150 + b"CCG" * 50
    return mk.base(tr=long_, reads=[mk.read(short if i % 2 else long_) for i in range(300)])


def case_purity(mk):
    """case 11: read qualities >= 0.9, < 0.9 and None; some reads carry an impure insert; a clean deep locus and a shallow one beside"""
    rq = lambda n: [None if i % 5 == 0 else (0.95 if i % 5 < 3 else 0.5) for i in range(n)]
    impure = lambda rep: rep[:9] + b"TTGATTCA" + rep[17:]
    het = mk.het(300, 0.03)
    het["reads"] = [mk.read(impure(B)) if i % 23 == 0 else r for i, r in enumerate(het["reads"])]
    clean = mk.het(400)
    clean["reads"] = [mk.read(impure(A)) if i % 31 == 0 else r for i, r in enumerate(clean["reads"])]
    return [dict(het, read_qual=rq(300)), dict(clean, read_qual=rq(400)), dict(mk.het(90, 0.03), read_qual=rq(90))]


def test_clean_heterozygous_257_600_1100(oracle, locus, deep_ctx):
    # case 1: the first size beyond the one-wave envelope, and sizes that take several passes of every workgroup-wide loop
    mk = Maker(201)
    b, refs = _check(oracle, locus, [mk.het(257), mk.het(600), mk.het(1100)], locus.Params(**DEEP), deep_ctx, (3, 0, 0))
    assert all(r["stats"]["n_wfa_cons"] == 0 for r in refs)


def test_noisy_heterozygous_300_600(oracle, locus, deep_ctx):
    # case 2: most segments are unique, the picks lack majority support, the repair runs
    mk = Maker(202)
    b, refs = _check(oracle, locus, [mk.het(300, 0.03), mk.het(600, 0.03)], locus.Params(**DEEP), deep_ctx, (2, 2, 0))
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs)


def test_default_cli_depth(oracle, locus, deep_ctx):
    # case 3: Params() as the command line leaves them: max_depth 250, the oracle keeps 250 reads of 300 and of 750
    mk = Maker(203)
    loci = [mk.het(300), mk.het(750), mk.het(300, 0.03), mk.het(750, 0.03)]
    params = locus.Params()
    assert params.max_depth == 250
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    assert [len(r["kept_read"]) for r in refs] == [250] * 4
    assert _repaired(b, refs) == 2
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert deep_ctx.size_deep_stats() == (4, 2, 0, 0), mode


def test_downsample_keeps_more_than_256(oracle, locus, deep_ctx):
    # case 4: 600 reads, max_depth = 270
    mk = Maker(204)
    loci = [mk.het(600, 0.03)]
    params = locus.Params(max_depth=270)
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    assert 256 < len(refs[0]["kept_read"]) < 600
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert deep_ctx.size_deep_stats() == (1, _repaired(b, refs), 0, 0), mode


def test_ceiling(oracle, locus, deep_ctx, limit):
    # case 5: exactly `limit` reads is the device chain's; one more is outside the setting and the host path's
    mk = Maker(205)
    _check(oracle, locus, [mk.het(limit)], locus.Params(**DEEP), deep_ctx, (1, 0, 0))
    _check(oracle, locus, [mk.het(limit + 1)], locus.Params(**DEEP), deep_ctx, (0, 0, 0))


def test_haploid_300(oracle, locus, deep_ctx):
    # case 6
    mk = Maker(206)
    loci = [mk.base(ploidy=1, reads=[mk.read(B) for _ in range(300)]), mk.base(ploidy=1, reads=[mk.read(mk.noisy(B)) for _ in range(300)])]
    b, refs = _check(oracle, locus, loci, locus.Params(**DEEP), deep_ctx, (2, 1, 0))
    assert refs[0]["stats"]["n_wfa_cons"] == 0 and refs[1]["stats"]["n_wfa_cons"] > 0


def test_homozygous_400_identical_segments(oracle, locus, deep_ctx):
    # case 7: every length difference ties, the tie-breaker alternates over all kept reads
    mk = Maker(207)
    b, refs = _check(oracle, locus, [mk.base(reads=[mk.read(A) for _ in range(400)])], locus.Params(**DEEP), deep_ctx, (1, 0, 0))
    cls = refs[0]["classification"].tolist()
    assert len(cls) == 400 and all(cls[i] != cls[i + 1] for i in range(399))


def test_many_unique_lengths(oracle, locus, deep_ctx):
    # case 8: 150 unique lengths, 11 325 diploid candidates (44 or 45 per thread); the mirrored histogram has its smallest penalty twice
    mk = Maker(208)
    loci = [case_many_lengths(mk, False), case_many_lengths(mk, True)]
    params = locus.Params(**DEEP)
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    for l in range(2):
        a0 = int(b["locus_read_begin"][l])
        lens = [int(refs[l]["span_end"][r] - refs[l]["span_start"][r]) for r in refs[l]["kept_read"].tolist()]
        assert 380 < len(lens) < 420 and len(set(lens)) == 150, (len(lens), len(set(lens)), a0)
    pens = diploid_penalties(lens)  # (of the mirrored locus)
    best = min(pens.values())
    tied = sorted(p for p, v in pens.items() if v == best)
    assert len(tied) >= 2, tied  # the first candidate in (short, long) order must win
    assert sorted(len(s) for s in refs[1]["alleles"]) == list(tied[0])
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert deep_ctx.size_deep_stats() == (2, _repaired(b, refs), 0, 0), mode


def test_collapse_to_one_length(oracle, locus, deep_ctx):
    # case 9: top_frac > 0.6 and range <= 6
    mk = Maker(209)
    b = locus.pack([case_collapse(mk)])
    params = locus.Params(**DEEP)
    refs = _refs(oracle, b, params)
    assert refs[0]["n_alleles"] == 2 and refs[0]["alleles"][0] == refs[0]["alleles"][1]
    assert len(set(int(refs[0]["span_end"][r] - refs[0]["span_start"][r]) for r in refs[0]["kept_read"].tolist())) == 7
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert deep_ctx.size_deep_stats() == (1, _repaired(b, refs), 0, 0), mode


def test_reference_allele_first_long_segments(oracle, locus, deep_ctx):
    # case 10: 300 segments of 540 and 600 bases (168 KB: beyond any LDS staging); the longer allele is the reference and comes first
    mk = Maker(210)
    L = case_long_reference_first(mk)
    b, refs = _check(oracle, locus, [L], locus.Params(**DEEP), deep_ctx, (1, 0, 0))
    ref = refs[0]
    assert [len(s) for s in ref["alleles"]] == [600, 540] and ref["alleles"][0].encode() == L["tr"]  # flipped: the size genotyper orders short, long
    assert sum(int(ref["span_end"][r] - ref["span_start"][r]) for r in ref["kept_read"].tolist()) > 160 * 1024


def test_purity_filter_on(oracle, locus, deep_ctx):
    # case 11: filter_impure_trs on; the deep and the shallow selection append to one purity job list
    mk = Maker(211)
    loci = case_purity(mk)
    for params in (locus.Params(min_read_qual=-1.0, **DEEP), locus.Params(min_read_qual=-1.0)):
        b = locus.pack(loci)
        refs = _refs(oracle, b, params)
        for mode, out in _runs(locus, b, params, deep_ctx):
            _compare(locus, b, out, refs)
            assert deep_ctx.size_deep_stats() == (2, _repaired(b, refs), 0, 0), (mode, params.max_depth)


def test_mixed_batch(oracle, locus, limit):
    # case 12: shallow size loci of both one-wave instantiations, a deep size locus, a shallow and a deep cluster locus in one call
    _lib = _lib_mod()
    mk = Maker(212)
    loci = [mk.het(12), mk.cluster_het(40), mk.het(64, 0.03), mk.het(256), mk.cluster_het(300), mk.het(270, 0.03)]
    params = locus.Params(**DEEP)
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    both, size_only = _lib.Context(0), _lib.Context(0)
    try:
        both.set_size_max_reads(limit)
        both.set_cluster_max_reads(_lib.cluster_max_reads_limit())
        size_only.set_size_max_reads(limit)
        for ctx, n_cluster in ((both, 2), (size_only, 1)):
            for mode, out in _runs(locus, b, params, ctx):
                _compare(locus, b, out, refs)
                assert ctx.size_deep_stats() == (1, _repaired(b, refs), 0, 0), mode
                assert int(out.stats[22]) == n_cluster and int(out.stats[23]) == 0, (mode, out.stats[22:24])
    finally:
        both.close()
        size_only.close()


def test_boundary_of_the_setting(oracle, locus, limit):
    # case 13: set to 300, a locus of 300 reads is the device chain's, one of 301 the host path's; the setter's bounds; the default
    _lib = _lib_mod()
    mk = Maker(213)
    ctx = _lib.Context(0)
    try:
        L = _lib.lib()
        params = locus.Params(**DEEP)
        b = locus.pack([mk.het(280, 0.03)])
        refs = _refs(oracle, b, params)
        out = locus.run_batch(b, params, ctx=ctx)  # the default: today's behaviour
        _compare(locus, b, out, refs)
        assert ctx.size_deep_stats() == (0, 0, 0, 0)
        ctx.set_size_max_reads(300)
        for bad in (255, limit + 1, 0, -1):
            assert L.trgt_hip_set_size_max_reads(ctx.handle, bad) == -1  # TRGT_ERR_INVALID
            assert b"trgt_hip_set_size_max_reads" in L.trgt_hip_last_error(ctx.handle)
            with pytest.raises(_lib.TrgtHipError):
                ctx.set_size_max_reads(bad)
        # (refused: the setting is still 300)
        _check(oracle, locus, [mk.het(300, 0.03), mk.het(301, 0.03)], params, ctx, (1, 1, 0))
        out = locus.run_batch(b, params, ctx=ctx)
        _compare(locus, b, out, refs)
        assert ctx.size_deep_stats() == (1, 1, 0, 0)
    finally:
        ctx.close()


def test_handed_back_to_the_host(oracle, locus, limit):
    # case 14: the repair takes segments of at most 40 bases here, the 51-base allele's group cannot join it: the host path, same results
    _lib = _lib_mod()
    mk = Maker(214)
    ctx = _lib.context_with_env(TRGT_REPAIR_MAX_SEG=40)
    try:
        ctx.set_size_max_reads(limit)
        b, refs = _check(oracle, locus, [mk.het(300, 0.03)], locus.Params(**DEEP), ctx, (0, 0, 1))
        assert refs[0]["stats"]["n_wfa_cons"] > 0
    finally:
        ctx.close()


def test_pool_of_two_contexts(oracle, locus, deep_ctx, limit):
    # case 15: four batches holding deep size loci through a pool whose contexts are both set: the one-context results
    _lib = _lib_mod()
    mk = Maker(215)
    params = locus.Params(**DEEP)
    batches = [locus.pack([mk.het(270 + 10 * k, 0.03), mk.het(20 + k), mk.het(300)]) for k in range(4)]
    single = [locus.run_batch(b, params, ctx=deep_ctx) for b in batches]
    assert deep_ctx.size_deep_stats()[0] == 2
    pool = _lib.Pool([0, 0], size_max_reads=limit)
    try:
        outs, ran = locus.run_many(pool, batches, params)
    finally:
        pool.close()
    assert sorted(set(ran)) <= [0, 1]
    for b, one, many in zip(batches, single, outs):
        for name in ("span_start", "span_end", "n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "n_spans", "motif_counts"):
            assert np.array_equal(getattr(one, name), getattr(many, name)), name
        assert int(one.stats[18]) == int(many.stats[18]) == 1  # (the noisy deep locus went through the device-side repair in both)
        for l in range(3):
            assert locus.locus_result(b, one, l) == locus.locus_result(b, many, l)
    _compare(locus, batches[0], outs[0], _refs(oracle, batches[0], params))
