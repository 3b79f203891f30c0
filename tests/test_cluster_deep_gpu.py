"""Genotyper::Cluster loci deeper than 256 reads on the device (locus_cluster_deep.hpp, opt-in per context through
trgt_hip_set_cluster_max_reads): parity with the CPU oracle's restatement of analyze_tr -- spans, alleles, kept reads and their order,
classification, AL / ALLR / SD / MC / MS / AP -- with host reads and with reads resident in HBM, for every branch of
genotype_cluster::genotype at these depths, the planner's boundaries and the setter itself.

Loci are hand-made like those of test_locus_gpu.py::test_cluster_genotyper_shapes: 250-base flanks and repeat segments of 24-60 bases,
so that every pair of segments is aligned (|a| * |b| <= MAX_OPS) unless a case says otherwise.  The oracle's result of a locus is
computed once and compared with both runs."""
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
    return _lib_mod().cluster_max_reads_limit()


@pytest.fixture(scope="module")
def deep_ctx(limit):
    ctx = _lib_mod().Context(0)
    ctx.set_cluster_max_reads(limit)
    yield ctx
    ctx.close()


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
        return dict(dict(left_flank=self.lf, right_flank=self.rf, motifs=[b"CAG", b"CCG"], genotyper="cluster", tr=b"CAG" * 8), **kw)

    def het(self, n, **kw):
        return self.base(reads=[self.read(self.noisy(b"CAG" * 8 + b"CCG" * (3 if i % 2 else 9))) for i in range(n)], **kw)


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


def _check(oracle, locus, loci, params, ctx, n_deep=None, refs_out=None):
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    if refs_out is not None:
        refs_out.extend(refs)
    for mode, out in _runs(locus, b, params, ctx):
        _compare(locus, b, out, refs)
        if n_deep is not None:
            assert int(out.stats[22]) == n_deep and int(out.stats[23]) == 0, (mode, out.stats[22:24])
    return b, refs


DEEP = dict(max_depth=10000)


def test_heterozygous_257_600_1100(oracle, locus, deep_ctx):
    # case 1: the first size beyond the one-wave envelope, and sizes that take several passes of every workgroup-wide loop (256 threads)
    mk = Maker(101)
    loci = [mk.het(257), mk.het(600), mk.het(1100)]
    params = locus.Params(**DEEP)
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert int(out.stats[22]) == 3 and int(out.stats[23]) == 0 and int(out.stats[15]) > 0, (mode, out.stats[22:24], out.stats[15])


def test_downsample_in_front_of_the_pair_list(oracle, locus, deep_ctx):
    # case 2: 600 reads, max_depth = 270: the kept count is above 256 and below 600
    mk = Maker(102)
    params = locus.Params(max_depth=270)
    refs = []
    _check(oracle, locus, [mk.het(600)], params, deep_ctx, n_deep=1, refs_out=refs)
    assert 256 < len(refs[0]["kept_read"]) < 600


def test_haploid_300(oracle, locus, deep_ctx):
    # case 3
    mk = Maker(103)
    loci = [mk.base(ploidy=1, reads=[mk.read(mk.noisy(b"CAG" * 12)) for _ in range(300)])]
    _check(oracle, locus, loci, locus.Params(**DEEP), deep_ctx, n_deep=1)


def test_homozygous_400_identical_segments(oracle, locus, deep_ctx):
    # case 4: every distance ties at 0, the cut-off is 0, the even / odd split applies
    mk = Maker(104)
    loci = [mk.base(reads=[mk.read(b"CAG" * 11) for _ in range(400)])]
    refs = []
    _check(oracle, locus, loci, locus.Params(**DEEP), deep_ctx, n_deep=1, refs_out=refs)
    cls = refs[0]["classification"].tolist()
    assert len(cls) == 400 and all(cls[i] != cls[i + 1] for i in range(399))  # (the oracle took the even / odd branch)


def test_small_group_is_outlier_redo(oracle, locus, deep_ctx):
    # case 5: 380 + 40 reads nine bases apart and two stray reads: small_group_is_outlier asks for the even / odd redo -- a second
    # consensus round over all kept reads, which the oracle counts
    mk = Maker(105)
    reads = [mk.read(b"CAG" * 10) for _ in range(380)] + [mk.read(b"CAG" * 13) for _ in range(40)] + [mk.read(mk.noisy(b"CAG" * 20)), mk.read(mk.dna(24))]
    refs = []
    _check(oracle, locus, [mk.base(reads=reads)], locus.Params(**DEEP), deep_ctx, n_deep=1, refs_out=refs)
    assert refs[0]["stats"]["n_wfa_cons"] == 2 * len(refs[0]["kept_read"])


def _three_groups(mk):
    a, bq, far = b"CAG" * 8, b"CAG" * 9, mk.dna(150)
    reads = [mk.read(mk.noisy(a, 0.01)) for _ in range(200)] + [mk.read(mk.noisy(bq, 0.01)) for _ in range(150)] + [mk.read(mk.noisy(far, 0.01)) for _ in range(3)]
    order = mk.rng.permutation(len(reads))
    return [reads[i] for i in order], [int(i) for i in order]


def test_dropped_reads_go_to_the_closer_allele(oracle, locus, deep_ctx):
    # case 6: three well separated groups of 200 / 150 / 3 reads, the third far from both.  A third group is only dropped by cluster()
    # when it is smaller than min_cluster_size = max(2, round(0.01 n)) -- 4 here, the term that first matters at these depths; a group of
    # 30 would need 3 000 reads -- and far enough for its Ward merge to come after the merge of the two alleles.  The three reads are
    # then assigned by their edit distances to both alleles.
    mk = Maker(106)
    reads, order = _three_groups(mk)
    refs = []
    _check(oracle, locus, [mk.base(reads=reads)], locus.Params(**DEEP), deep_ctx, n_deep=1, refs_out=refs)
    ref = refs[0]
    third = [k for k, r in enumerate(ref["kept_read"]) if order[int(r)] >= 350]
    assert len(third) == 3 and len(ref["kept_read"]) == 353
    assert ref["stats"]["n_wfa_cons"] == 350  # (the oracle took that branch: three reads were in neither consensus group ...)
    assert ref["stats"]["n_wfa_ed"] == 353 * 352 // 2 - 3 + 6  # (... and were aligned to both alleles; the 150-base reads exceed MAX_OPS among themselves)
    assert [int(ref["classification"][k]) for k in third] == [1, 1, 1]  # closer to the 27-base allele by three bases: no tie to break


def test_max_ops_shortcut_for_every_pair(oracle, locus, deep_ctx):
    # case 7: alleles of 180 and 225 bases: |a| * |b| > MAX_OPS for every pair, the matrix is all length differences
    mk = Maker(107)
    loci = [mk.base(tr=b"CAG" * 60, reads=[mk.read(mk.noisy(b"CAG" * (60 if i % 2 else 75), 0.01)) for i in range(300)])]
    refs = []
    _check(oracle, locus, loci, locus.Params(**DEEP), deep_ctx, n_deep=1, refs_out=refs)
    assert refs[0]["stats"]["n_wfa_ed"] == 0


def test_mixed_batch(oracle, locus, deep_ctx):
    # case 8: size loci, shallow cluster loci of both one-wave instantiations and deep cluster loci in one call
    mk = Maker(108)
    loci = [
        mk.base(genotyper="size", reads=[mk.read(b"CAG" * (8 if i % 2 else 10)) for i in range(12)]),
        mk.het(40), mk.het(300), mk.het(130),
        mk.base(genotyper="size", reads=[mk.read(b"CAG" * (9 if i % 3 else 12)) for i in range(270)]),
        mk.base(ploidy=1, reads=[mk.read(mk.noisy(b"CAG" * 9)) for _ in range(260)]),
        mk.het(64), mk.het(256),
    ]
    params = locus.Params(**DEEP)
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    n_cluster = sum(1 for L in loci if L["genotyper"] == "cluster")
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert int(out.stats[22]) == n_cluster and int(out.stats[23]) == 0, (mode, out.stats[22:24])


def test_purity_filter_on(oracle, locus, deep_ctx):
    # case 9: the deep shapes with filter_impure_trs on (min_read_qual = -1.0, the targeted preset) and read qualities >= 0.9, < 0.9, NaN
    mk = Maker(109)
    rq = lambda n: [None if i % 5 == 0 else (0.95 if i % 5 < 3 else 0.5) for i in range(n)]
    impure = lambda rep: rep[:9] + b"TTGATTCA" + rep[17:]
    het = mk.het(300)
    het["reads"] = [mk.read(impure(b"CAG" * 8 + b"CCG" * 9)) if i % 23 == 0 else r for i, r in enumerate(het["reads"])]
    loci = [
        dict(het, read_qual=rq(300)),
        dict(mk.base(ploidy=1, reads=[mk.read(mk.noisy(b"CAG" * 12, 0.05)) for _ in range(280)]), read_qual=rq(280)),
        dict(mk.base(reads=[mk.read(b"CAG" * 11) for _ in range(400)]), read_qual=rq(400)),
        dict(mk.het(90), read_qual=rq(90)),
        dict(mk.het(600), read_qual=[None] * 600),
    ]
    params = locus.Params(min_read_qual=-1.0, **DEEP)
    _check(oracle, locus, loci, params, deep_ctx, n_deep=5)
    params = locus.Params(min_read_qual=-1.0, max_depth=270)
    _check(oracle, locus, [loci[4]], params, deep_ctx, n_deep=1)


def test_targeted_preset_scoring(oracle, locus, deep_ctx):
    # case 10: --preset targeted: scoring 1,0,1 and min_flank_id_frac 0.8
    mk = Maker(110)
    params = locus.Params(aln_scoring=(1, 0, 1), min_flank_id_frac=0.8, min_read_qual=-1.0, **DEEP)
    _check(oracle, locus, [mk.het(320)], params, deep_ctx, n_deep=1)


def test_boundary_of_the_setting(oracle, locus):
    # case 11: set to 300, a locus of 300 reads is the device chain's, one of 301 the host path's
    mk = Maker(111)
    ctx = _lib_mod().Context(0)
    try:
        ctx.set_cluster_max_reads(300)
        params = locus.Params(**DEEP)
        b = locus.pack([mk.het(300), mk.het(301)])
        refs = _refs(oracle, b, params)
        for mode, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs)
            assert int(out.stats[22]) == 1 and int(out.stats[23]) == 0, (mode, out.stats[22:24])
            assert int(out.read_rank[:300].max()) == 299
    finally:
        ctx.close()


def test_ceiling_and_room(oracle, locus, deep_ctx, limit):
    # case 12: one read beyond the ceiling: the host path, same results (long alleles: no pair is aligned, which keeps the oracle quick) ...
    mk = Maker(112)
    params = locus.Params(**DEEP)
    loci = [mk.base(tr=b"CAG" * 60, reads=[mk.read(mk.noisy(b"CAG" * (60 if i % 2 else 75), 0.01)) for i in range(limit + 1)])]
    b = locus.pack(loci)
    refs = _refs(oracle, b, params)
    for mode, out in _runs(locus, b, params, deep_ctx):
        _compare(locus, b, out, refs)
        assert int(out.stats[22]) == 0 and int(out.stats[23]) == 0, (mode, out.stats[22:24])
    # ... and a call whose deep loci do not all find room: small arenas and a small budget send some to the host path, none fails the call
    actx = _lib_mod().context_with_env(TRGT_CLUSTER_ARENA_KB=200)
    try:
        actx.set_cluster_max_reads(limit)
        loci = [mk.het(300) for _ in range(6)]
        b = locus.pack(loci)
        refs = _refs(oracle, b, params)
        for mode, out in _runs(locus, b, params, actx):
            _compare(locus, b, out, refs)
            assert 0 < int(out.stats[22]) < 6 and int(out.stats[23]) > 0, (mode, out.stats[22:24])
    finally:
        actx.close()


def test_setter_bounds(oracle, locus, limit):
    # case 13
    _lib = _lib_mod()
    mk = Maker(113)
    ctx = _lib.Context(0)
    try:
        L = _lib.lib()
        for bad in (255, limit + 1, 0, -1):
            assert L.trgt_hip_set_cluster_max_reads(ctx.handle, bad) == -1  # TRGT_ERR_INVALID
            assert b"trgt_hip_set_cluster_max_reads" in L.trgt_hip_last_error(ctx.handle)
            with pytest.raises(_lib.TrgtHipError):
                ctx.set_cluster_max_reads(bad)
        params = locus.Params(**DEEP)
        b = locus.pack([mk.het(280), mk.het(30)])
        refs = _refs(oracle, b, params)
        out = locus.run_batch(b, params, ctx=ctx)  # the setting is still the default: the deep locus is the host path's
        _compare(locus, b, out, refs)
        assert int(out.stats[22]) == 1
        ctx.set_cluster_max_reads(limit)
        ctx.set_cluster_max_reads(256)
        out = locus.run_batch(b, params, ctx=ctx)
        assert int(out.stats[22]) == 1
        ctx.set_cluster_max_reads(limit)
        assert L.trgt_hip_set_cluster_max_reads(ctx.handle, 255) == -1  # (refused: the setting stays at the limit)
        out = locus.run_batch(b, params, ctx=ctx)
        _compare(locus, b, out, refs)
        assert int(out.stats[22]) == 2
    finally:
        ctx.close()


def test_pool_of_two_contexts(oracle, locus, deep_ctx, limit):
    # case 14: four batches holding deep loci through a pool whose contexts are both set: the one-context results
    _lib = _lib_mod()
    mk = Maker(114)
    params = locus.Params(**DEEP)
    batches = [locus.pack([mk.het(270 + 10 * k), mk.het(20 + k), mk.het(300)]) for k in range(4)]
    single = [locus.run_batch(b, params, ctx=deep_ctx) for b in batches]
    pool = _lib.Pool([0, 0], cluster_max_reads=limit)
    try:
        outs, ran = locus.run_many(pool, batches, params)
    finally:
        pool.close()
    assert sorted(set(ran)) <= [0, 1]
    for b, one, many in zip(batches, single, outs):
        assert int(one.stats[22]) == 3 and int(many.stats[22]) == 3
        for name in ("span_start", "span_end", "n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "n_spans", "motif_counts"):
            assert np.array_equal(getattr(one, name), getattr(many, name)), name
        for l in range(3):
            assert locus.locus_result(b, one, l) == locus.locus_result(b, many, l)
    _compare(locus, batches[0], outs[0], _refs(oracle, batches[0], params))
