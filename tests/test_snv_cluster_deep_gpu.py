"""The SNV branch of genotype_flank (get_trs_with_clustering, genotype_flank.rs:78-138, 171-290; applied by analyze at tr.rs:64-75) for
Genotyper::Cluster loci of 257 to 2 048 candidate reads, behind the deep cluster chain: the SNV forms of
trgt_amd/csrc/locus_cluster_flank_deep.hpp, opt-in per context through trgt_hip_set_snv_cluster_deep_device on a context that also has
trgt_hip_set_cluster_max_reads.

Every case compares alleles, kept reads and their order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS /
AP with the oracle's restatement of analyze_tr, for five contexts -- the new setting with cluster_max_reads; that plus
flank_cluster_deep_device; every setting on; cluster_max_reads alone; a context as it is created -- and with the reads on the host and
resident in HBM; `flipped`, which the oracle does not report, must agree between them.  The results are the host redo's on the last two
contexts: what fails without the route are the statistics, which tests/snv_cluster_deep_cases.py computes from the oracle's plain result
and the restatement of get_trs_with_clustering, never from the library.  The conditions of the cases themselves are asserted without a
GPU in tests/test_snv_cluster_deep_cases.py."""
import numpy as np
import pytest

import snv_cluster_deep_cases as sc
from test_flank_device_gpu import _compare, _ref, _runs
from test_snv_cluster_deep_cases import no_room_arithmetic

pytestmark = pytest.mark.gpu
ZERO, ZERO3 = sc.ZERO, (0, 0, 0)
ROUTE = ("deep snv", "deep snv and tags", "all settings")
TAG_ROUTE = ("deep snv and tags", "all settings")


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def limit():
    from trgt_amd import _lib
    return _lib.cluster_max_reads_limit()


def _every(ctx, limit):
    ctx.set_cluster_max_reads(limit); ctx.set_size_max_reads(limit)
    for name in ("flank", "snv_split", "flank_cluster", "snv_cluster", "flank_cluster_deep", "snv_cluster_deep"):
        getattr(ctx, "set_%s_device" % name)(True)


@pytest.fixture(scope="module")
def ctxs(limit):
    from trgt_amd import _lib
    on, both, every, deep, plain = (_lib.Context(0) for _ in range(5))
    on.set_cluster_max_reads(limit); on.set_snv_cluster_deep_device(True)
    both.set_cluster_max_reads(limit); both.set_snv_cluster_deep_device(True); both.set_flank_cluster_deep_device(True)
    _every(every, limit)
    deep.set_cluster_max_reads(limit)
    yield [("deep snv", on), ("deep snv and tags", both), ("all settings", every), ("deep chain only", deep), ("plain", plain)]
    for c in (on, both, every, deep, plain):
        c.close()


def _check(oracle, locus, ctxs, loci, kw=None, handed=(), want=None, want_tags=None, only=None, max_reads=sc.CEILING, name="deep snv"):
    """want / want_tags: what the case itself expects of the two deep statistics (checked against the restatement before any GPU run);
    only: one context (set like the one of ctxs called `name`) instead of the five"""
    params = locus.Params(**(kw or {}))
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = sc.plain_results(oracle, loci, params)
    stats, tags = sc.expected_stats(loci, plain, max_reads, handed), sc.tag_stats(loci, plain, max_reads)
    if want is not None:
        assert stats == want
    if want_tags is not None:
        assert tags == want_tags
    flipped, outs = [], []
    for name, ctx in ([(name, only)] if only is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            expect = stats if name in ROUTE else ZERO
            print(name, how, "snv_cluster_deep_stats", ctx.snv_cluster_deep_stats(), "expected", expect, "flank_cluster_deep_stats", ctx.flank_cluster_deep_stats())
            assert ctx.snv_cluster_deep_stats() == expect, (name, how)
            # the older routes' counts stay untouched by these loci
            assert ctx.flank_cluster_deep_stats() == (tags if name in TAG_ROUTE else ZERO3), (name, how)
            if name != "all settings":
                assert ctx.snv_cluster_stats() == ZERO and ctx.flank_cluster_stats() == ZERO3 and ctx.flank_stats() == ZERO and ctx.snv_split_stats() == ZERO, (name, how)
            outs.append((name, how, out))
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, plain, outs


def test_default_depth_keeps_250_of_257(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_default_depth(), {}, want=(1, 0, 0, 0))


def test_depths_and_rounds_of_the_workgroup(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_depths(), sc.DEEP, want=(3, 0, 0, 0))


@pytest.mark.parametrize("n", sorted(sc.SKIPS))
def test_skip_rounding_and_the_edges_of_the_region(oracle, locus, ctxs, n):
    _check(oracle, locus, ctxs, sc.case_skip(n)[0], sc.DEEP, want=(2, 0, 0, 0))


def test_ties_across_the_round_boundary(oracle, locus, ctxs):
    _, refs, plain, _ = _check(oracle, locus, ctxs, sc.case_ties(), sc.DEEP, want=(1, 1, 0, 0))
    # the third round got two jobs for each tied read: 75 members of the repaired group 0
    assert refs[0]["stats"]["n_wfa_cons"] - plain[0]["stats"]["n_wfa_cons"] == 70 + sc.N_TIES


def test_margin(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_margin(), sc.DEEP, want=(1, 0, 0, 2))


def test_repair_swap_flip_and_no_split(oracle, locus, ctxs):
    _, refs, _, outs = _check(oracle, locus, ctxs, sc.case_repair(), sc.DEEP, want=(4, 2, 0, 0))
    assert all([int(v) for v in out.flipped[2:4]] == [0, 1] for _, _, out in outs)


def test_limits_snvs_and_profiles(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_snv_cap(), sc.DEEP, want=(1, 0, 1, 0))
    _check(oracle, locus, ctxs, sc.case_hap_cap(), sc.DEEP, want=(1, 0, 1, 0))


def test_limit_of_in_region_offsets_at_the_ceiling(oracle, locus, ctxs):
    on = dict(ctxs)["deep snv"]
    _check(oracle, locus, ctxs, sc.case_offset_cap(), sc.DEEP, want=(1, 0, 1, 0), only=on)


def test_tags_and_snvs(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_tags_and_snvs(), sc.DEEP, want=(2, 0, 0, 0), want_tags=(1, 0, 0))


def test_tag_locus_and_snv_locus_share_the_third_round(oracle, locus, ctxs):
    _, refs, plain, _ = _check(oracle, locus, ctxs, sc.case_tags_and_snvs_repaired(), sc.DEEP, want=(1, 1, 0, 0), want_tags=(1, 1, 0))
    assert all(r["stats"]["n_wfa_cons"] > q["stats"]["n_wfa_cons"] > 0 for r, q in zip(refs, plain))


def test_no_room_for_the_third_round_hands_the_locus_back(oracle, locus, ctxs, limit):
    from trgt_amd import _lib
    kb = no_room_arithmetic()
    loci = sc.case_no_room()
    ctx = _lib.context_with_env(TRGT_CLUSTER_ARENA_KB=kb)
    try:
        ctx.set_cluster_max_reads(limit); ctx.set_snv_cluster_deep_device(True)
        _, _, _, outs = _check(oracle, locus, ctxs, loci, sc.DEEP, handed=(0,), want=(0, 0, 1, 0), only=ctx)
        assert all(int(out.stats[22]) == 1 and int(out.stats[23]) == 0 for _, _, out in outs)
    finally:
        ctx.close()
    _check(oracle, locus, ctxs, loci, sc.DEEP, want=(1, 1, 0, 0), only=dict(ctxs)["deep snv"])  # with room, the same locus is repaired on the device


def test_allele_beyond_allele_cap_hands_the_locus_back(oracle, locus, ctxs):
    """the chain's own alleles (60 / 60) fit the buffer, the SNV split's (63) does not: the route hands the locus back, and the host path
    reports the error as it does without the setting (as behind the one-wave chain, tests/test_snv_cluster_gpu.py)"""
    from trgt_amd import _lib
    loci = sc.case_allele_cap()
    params = locus.Params(**sc.DEEP)
    b = locus.pack(loci)
    plain = sc.plain_results(oracle, loci, params)
    refs = [_ref(oracle, L, params) for L in loci]
    assert sc.expected_stats(loci, plain) == (1, 0, 0, 0) and sc.expected_stats(loci, plain, handed=(0,)) == (0, 0, 1, 0)
    for name, ctx in ctxs:
        small = locus.BatchOutputs(b)
        small.allele_cap[:] = sc.ALLELE_CAP
        with pytest.raises(_lib.TrgtHipError, match="allele_cap"):
            locus.run_batch(b, params, ctx, outputs=small)
        assert ctx.snv_cluster_deep_stats() == ((0, 0, 1, 0) if name in ROUTE else ZERO), name
        _compare(locus, b, locus.run_batch(b, params, ctx), refs, (name, "the context is still usable"))
        assert ctx.snv_cluster_deep_stats() == ((1, 0, 0, 0) if name in ROUTE else ZERO), name


@pytest.mark.parametrize("kw", [dict(sc.PURITY, **sc.DEEP)])
def test_purity_filter_on(oracle, locus, ctxs, kw):
    _check(oracle, locus, ctxs, sc.case_purity(), kw, want=(2, 0, 0, 0))


def test_mixed_batch_keeps_the_settings_apart(oracle, locus, ctxs, limit):
    from trgt_amd import _lib
    loci = sc.case_mixed()
    ctx = _lib.Context(0)
    try:
        _every(ctx, limit); ctx.set_cluster_max_reads(sc.MIXED_SETTING)
        _, _, plain, outs = _check(oracle, locus, ctxs, loci, sc.DEEP, want=(1, 0, 0, 0), want_tags=ZERO3, only=ctx, max_reads=sc.MIXED_SETTING, name="all settings")
        import snv_cluster_cases as shallow
        import snv_deep_cases as size
        assert ctx.snv_cluster_stats() == shallow.expected_stats(loci, plain) == (1, 0, 0, 0)
        assert ctx.snv_split_stats() == size.expected_stats(loci, plain)[0] == (2, 0, 0, 0)
    finally:
        ctx.close()
    _check(oracle, locus, ctxs, loci, sc.DEEP, want=(2, 0, 0, 0))  # at the ceiling the 301-read locus is the route's too


def test_setting_off_beside_the_one_wave_setting(oracle, locus, ctxs, limit):
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    try:
        ctx.set_cluster_max_reads(limit); ctx.set_snv_cluster_device(True)
        loci = sc.case_depths()
        params = locus.Params(**sc.DEEP)
        b = locus.pack(loci)
        refs = [_ref(oracle, L, params) for L in loci]
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, ("setting off", how))
            assert ctx.snv_cluster_deep_stats() == ZERO and ctx.snv_cluster_stats() == (2, 0, 0, 0), how
    finally:
        ctx.close()


def test_random_loci(oracle, locus, ctxs):
    on, deep = dict(ctxs)["deep snv"], dict(ctxs)["deep chain only"]
    loci = sc.case_random()
    params = locus.Params(**sc.DEEP)
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = sc.plain_results(oracle, loci, params)
    stats = sc.expected_stats(loci, plain)
    for name, ctx in (("deep snv", on), ("deep chain only", deep)):
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            assert ctx.snv_cluster_deep_stats() == (stats if ctx is on else ZERO), (name, how)


def test_other_entry_points(oracle, locus, ctxs, limit):
    """submit / wait, split batches, a pool created with the setting, and the setting on a batch without mismatch lists"""
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = dict(ctxs)["deep snv"]
    loci = sc.case_repair()[:3] + sc.case_depths()[3:]
    params = locus.Params(**sc.DEEP)
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, sc.DEEP, only=on, want=(3, 2, 0, 0))
    stats = sc.expected_stats(loci, plain)
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, params, ctx=on))
    assert recs(b, locus.submit_batch(b, params, ctx=on).wait()) == want and on.snv_cluster_deep_stats() == stats
    got, total = [], [0, 0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, params, ctx=on))
        total = [x + y for x, y in zip(total, on.snv_cluster_deep_stats())]
    assert got == want and tuple(total) == stats
    pool = _lib.Pool([0, 0], cluster_max_reads=limit, snv_cluster_deep_device=True)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks, params)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
        assert tuple(sum(c.snv_cluster_deep_stats()[i] for c in pool.contexts) for i in range(4)) != ZERO  # (the contexts' last calls: the route ran in the pool)
    finally:
        pool.close()
    # the setting on a batch without read metadata: the deep chain's genotype stands, nothing counted
    bare = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    _compare(locus, bare, locus.run_batch(bare, params, ctx=on, reads_dev=torch.from_numpy(bare["read_blob"]).cuda()), plain, "no mismatch lists")
    assert on.snv_cluster_deep_stats() == ZERO
