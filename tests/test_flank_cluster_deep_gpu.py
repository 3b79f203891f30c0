"""The haplotype-tag branch of genotype_flank (genotype_flank.rs:9-76, 147-170; applied by analyze at tr.rs:64-75 whichever genotyper
produced the alleles) for Genotyper::Cluster loci of 257 to 2 048 candidate reads, behind the deep cluster chain:
trgt_amd/csrc/locus_cluster_flank_deep.hpp, opt-in per context through trgt_hip_set_flank_cluster_deep_device on a context that also has
trgt_hip_set_cluster_max_reads.

Every case compares alleles, kept reads and their order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS /
AP with the oracle's restatement of analyze_tr, for four contexts -- the new setting with cluster_max_reads; that plus the two settings of
the one-wave cluster chain; cluster_max_reads alone; a context as it is created -- and with the reads on the host and resident in HBM;
`flipped`, which the oracle does not report, must agree between them.  The results are the host redo's on the last two contexts: what fails
without the route are the statistics, which tests/flank_cluster_deep_cases.py computes from the oracle's plain result and a restatement of
the tag rule, never from the library.  The conditions of the cases themselves are asserted without a GPU in
tests/test_flank_cluster_deep_cases.py.

The hand-back comes from the third round finding no room under TRGT_CLUSTER_ARENA_KB (the arithmetic is
test_flank_cluster_deep_cases.no_room_arithmetic, asserted there and here)."""
import numpy as np
import pytest

import flank_cluster_cases as shallow
import flank_cluster_deep_cases as fc
from test_flank_cluster_deep_cases import no_room_arithmetic
from test_flank_device_gpu import _compare, _ref, _runs

pytestmark = pytest.mark.gpu
ZERO = (0, 0, 0)
ROUTE = ("deep flank", "all settings")


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def limit():
    from trgt_amd import _lib
    return _lib.cluster_max_reads_limit()


@pytest.fixture(scope="module")
def ctxs(limit):
    from trgt_amd import _lib
    on, every, deep, plain = _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.Context(0)
    on.set_cluster_max_reads(limit); on.set_flank_cluster_deep_device(True)
    every.set_cluster_max_reads(limit); every.set_flank_cluster_deep_device(True); every.set_flank_cluster_device(True); every.set_snv_cluster_device(True)
    deep.set_cluster_max_reads(limit)
    yield [("deep flank", on), ("all settings", every), ("deep chain only", deep), ("plain", plain)]
    for c in (on, every, deep, plain):
        c.close()


def _check(oracle, locus, ctxs, loci, kw=None, handed=(), want=None, only=None, max_reads=fc.CEILING, name="deep flank"):
    """want: what the case itself expects of the statistics (checked against the restatement before any GPU run); only: one context (which
    has the route on; name: which of the four it is set like) instead of the four"""
    params = locus.Params(**(kw or {}))
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = fc.plain_results(oracle, loci, params)
    stats = fc.expected_stats(loci, plain, max_reads, handed)
    if want is not None:
        assert stats == want
    flipped, outs = [], []
    for name, ctx in ([(name, only)] if only is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            expect = stats if name in ROUTE else ZERO
            print(name, how, "flank_cluster_deep_stats", ctx.flank_cluster_deep_stats(), "expected", expect)
            assert ctx.flank_cluster_deep_stats() == expect, (name, how)
            if name != "all settings":
                assert ctx.flank_cluster_stats() == ZERO and ctx.flank_stats() == (0, 0, 0, 0), (name, how)
            outs.append((name, how, out))
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, plain, outs


def test_depths_and_rounds_of_the_workgroup(oracle, locus, ctxs):
    (one, kw1), (many, kw2) = fc.case_depths()
    _check(oracle, locus, ctxs, one, kw1, want=(1, 0, 0))
    _check(oracle, locus, ctxs, many, kw2, want=(4, 0, 0))


def test_the_ceiling(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_ceiling(), fc.DEEP, want=(1, 0, 0))


def test_tags_against_the_clusters(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_tags_against_clusters(), fc.DEEP, want=(1, 0, 0))


def test_homozygous_and_the_even_odd_redo(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_homozygous(), fc.DEEP, want=(2, 0, 0))


def test_acceptance_threshold_and_an_empty_group(oracle, locus, ctxs):
    assert 182.0 / 260.0 >= 0.7 and not 181.0 / 260.0 >= 0.7
    _check(oracle, locus, ctxs, fc.case_threshold(), fc.DEEP, want=(1, 0, 0))  # refused loci carry no mismatches: they stay on the device


def test_untagged_reads_alternate_across_the_rounds(oracle, locus, ctxs):
    _, refs, _, _ = _check(oracle, locus, ctxs, fc.case_boundary(), fc.DEEP, want=(1, 0, 0))
    assert refs[0]["alleles"] == [fc.X60.decode(), fc.W63.decode()]


def test_lexicographic_and_median_ties(oracle, locus, ctxs):
    _, refs, _, _ = _check(oracle, locus, ctxs, fc.case_ties(), fc.DEEP, want=(7, 2, 0))
    assert fc.CAA_CAG19.decode() in refs[0]["alleles"] and fc.CAA_CAG19.decode() in refs[1]["alleles"]
    assert fc.CAG20.decode() in refs[2]["alleles"] and fc.AAG_CAG19_CA.decode() in refs[3]["alleles"]


def test_noisy_groups_are_repaired_in_the_third_round(oracle, locus, ctxs):
    _, refs, plain, _ = _check(oracle, locus, ctxs, fc.case_repair(), fc.DEEP, want=(2, 2, 0))
    assert all(r["stats"]["n_wfa_cons"] > q["stats"]["n_wfa_cons"] > 0 for r, q in zip(refs, plain))


def test_reference_allele_first_after_the_swap(oracle, locus, ctxs):
    _, refs, _, outs = _check(oracle, locus, ctxs, fc.case_reference_first(), fc.DEEP, want=(2, 0, 0))
    assert refs[0]["alleles"] == [fc.CAG20.decode(), fc.CAG21.decode()] and refs[1]["alleles"] == [fc.CAG21.decode(), fc.CAG20.decode()]
    assert all([int(v) for v in out.flipped] == [0, 1] for _, _, out in outs)


@pytest.mark.parametrize("kw", [fc.PURITY, dict(fc.PURITY, **fc.DEEP)])
def test_purity_filter_on(oracle, locus, ctxs, kw):
    _check(oracle, locus, ctxs, fc.case_purity(), kw, want=(2, 0, 0))


def test_mixed_batch_keeps_the_settings_apart(oracle, locus, ctxs):
    loci = fc.case_mixed()
    params = locus.Params(**fc.DEEP)
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, fc.DEEP, want=(1, 0, 0))
    # every setting on: each count takes only its own loci -- the one-wave route's the two shallow cluster loci, this route's the deep one
    assert shallow.expected_stats(loci, plain) == (2, 0, 0)
    every = dict(ctxs)["all settings"]
    for how, out in _runs(locus, b, params, every):
        assert every.flank_cluster_stats() == (2, 0, 0) and every.flank_cluster_deep_stats() == (1, 0, 0) and every.flank_stats() == (0, 0, 0, 0), how
        assert every.snv_cluster_stats() == (0, 0, 0, 0), how
    # again at cluster_max_reads = 300, with a 301-read locus beside a 300-read one: the deep loci of the batch (300, 280, 270 reads) and the
    # 300-read locus are the deep chain's, the 301-read locus is the host's from the start and in no count
    from trgt_amd import _lib
    more = loci + fc.case_setting_300()
    ctx = _lib.Context(0)
    try:
        ctx.set_cluster_max_reads(300); ctx.set_flank_cluster_deep_device(True); ctx.set_flank_cluster_device(True)
        _, _, _, outs = _check(oracle, locus, ctxs, more, fc.DEEP, want=(2, 0, 0), only=ctx, max_reads=300, name="all settings")
        assert ctx.flank_cluster_stats() == (2, 0, 0)
        assert all(int(out.stats[22]) == 6 and int(out.stats[23]) == 0 for _, _, out in outs)  # five cluster loci of the batch and the 300-read one
    finally:
        ctx.close()


def test_a_setting_below_the_ceiling(oracle, locus, ctxs):
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    try:
        ctx.set_cluster_max_reads(300); ctx.set_flank_cluster_deep_device(True)
        _, _, _, outs = _check(oracle, locus, ctxs, fc.case_setting_300(), fc.DEEP, want=(1, 0, 0), only=ctx, max_reads=300)  # the 301-read locus is the host's
        assert all(int(out.stats[22]) == 1 and int(out.stats[23]) == 0 for _, _, out in outs)
    finally:
        ctx.close()


def test_the_setting_without_a_deep_chain_does_nothing(oracle, locus, ctxs):
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    try:
        ctx.set_flank_cluster_deep_device(True)  # (no set_cluster_max_reads: the setting has nothing to follow)
        loci = fc.case_setting_300()[:1]
        params = locus.Params(**fc.DEEP)
        b = locus.pack(loci)
        refs = [_ref(oracle, L, params) for L in loci]
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, ("no deep chain", how))
            assert ctx.flank_cluster_deep_stats() == ZERO and int(out.stats[22]) == 0, how
    finally:
        ctx.close()


def test_no_room_for_the_third_round_hands_the_locus_back(oracle, locus, ctxs, limit):
    from trgt_amd import _lib
    kb = no_room_arithmetic()  # admits the 257-read locus, fits round 1 (there is no second round), does not fit round 3
    loci = fc.case_no_room()
    ctx = _lib.context_with_env(TRGT_CLUSTER_ARENA_KB=kb)
    try:
        ctx.set_cluster_max_reads(limit); ctx.set_flank_cluster_deep_device(True)
        _, _, _, outs = _check(oracle, locus, ctxs, loci, fc.DEEP, handed=(0,), want=(0, 0, 1), only=ctx)
        for name, how, out in outs:
            assert int(out.stats[22]) == 1 and int(out.stats[23]) == 0, how
    finally:
        ctx.close()
    # with room, the same locus is repaired on the device
    _check(oracle, locus, ctxs, loci, fc.DEEP, want=(1, 1, 0), only=dict(ctxs)["deep flank"])


def test_other_entry_points(oracle, locus, ctxs, limit):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = dict(ctxs)["deep flank"]
    loci = fc.case_entry_points()
    params = locus.Params(**fc.DEEP)
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, fc.DEEP, only=on, want=(4, 1, 0))
    stats = fc.expected_stats(loci, plain)
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, params, ctx=on))
    assert recs(b, locus.submit_batch(b, params, ctx=on).wait()) == want and on.flank_cluster_deep_stats() == stats
    got, total = [], [0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, params, ctx=on))
        total = [x + y for x, y in zip(total, on.flank_cluster_deep_stats())]
    assert got == want and tuple(total) == stats
    pool = _lib.Pool([0, 0], cluster_max_reads=limit, flank_cluster_deep_device=True)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks, params)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
        assert tuple(sum(c.flank_cluster_deep_stats()[i] for c in pool.contexts) for i in range(3)) != ZERO  # (the contexts' last calls: the route ran in the pool)
    finally:
        pool.close()
    # the setting on a batch without hp_tag: the deep chain's genotype stands, nothing counted
    bare = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    _compare(locus, bare, locus.run_batch(bare, params, ctx=on, reads_dev=torch.from_numpy(bare["read_blob"]).cuda()), plain, "no hp_tag")
    assert on.flank_cluster_deep_stats() == ZERO
