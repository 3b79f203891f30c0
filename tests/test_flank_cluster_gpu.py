"""The haplotype-tag branch of genotype_flank (genotype_flank.rs:9-76, 147-170; applied by analyze at tr.rs:64-75 whichever genotyper
produced the alleles) behind the one-wave cluster chain: trgt_amd/csrc/locus_cluster_flank.hpp, opt-in per context through
trgt_hip_set_flank_cluster_device.

Every case compares alleles, kept reads and their order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS /
AP with the oracle's restatement of analyze_tr, for four contexts -- the setting on, the setting together with trgt_hip_set_flank_device, a
context as it is created, TRGT_HOST_CLUSTER=1 -- and with the reads on the host and resident in HBM; `flipped`, which the oracle does not
report, must agree between them.  The results are the host redo's on every context: what fails without the route are the statistics, which
tests/flank_cluster_cases.py computes from the oracle's plain result and a restatement of the tag rule.  The conditions of the cases
themselves are asserted without a GPU in tests/test_flank_cluster_cases.py."""
import numpy as np
import pytest

import flank_cluster_cases as fc
from test_flank_device_gpu import _compare, _expected_stats, _ref, _runs
from test_repair_needs import group_needs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def ctxs():
    from trgt_amd import _lib
    on, both, off, host = _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.context_with_env(TRGT_HOST_CLUSTER=1)
    on.set_flank_cluster_device(True)
    both.set_flank_cluster_device(True)
    both.set_flank_device(True)
    host.set_flank_cluster_device(True)  # (no device cluster chain: the setting has nothing to follow)
    yield [("on", on), ("both", both), ("off", off), ("host cluster", host)]
    for c in (on, both, off, host):
        c.close()


def _check(oracle, locus, ctxs, loci, params=None, handed=(), want=None, only=None):
    """want: what the case itself expects of the statistics (checked against the restatement before any GPU run); only: one context
    (which has the setting on) instead of the four"""
    params = params or locus.Params()
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = fc.plain_results(oracle, loci, params)
    stats = fc.expected_stats(loci, plain, handed)
    if want is not None:
        assert stats == want
    flipped, outs = [], []
    for name, ctx in ([("on", only)] if only is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            expect = stats if name in ("on", "both") else (0, 0, 0)
            print(name, how, "flank_cluster_stats", ctx.flank_cluster_stats(), "expected", expect)
            assert ctx.flank_cluster_stats() == expect, (name, how)
            if name in ("on", "off", "host cluster"):
                assert ctx.flank_stats() == (0, 0, 0, 0), (name, how)
            outs.append((name, how, out))
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, plain, outs


def test_het_and_reference_first(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_het(), want=(2, 0, 0))


def test_tags_against_the_clusters(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_tags_against_clusters(), want=(1, 0, 0))


def test_homozygous_and_the_even_odd_redo(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_homozygous(), want=(2, 0, 0))


def test_acceptance_threshold(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_threshold(), want=(1, 0, 0))


def test_loci_outside_the_route(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_no_route(), want=(1, 0, 0))


def test_lexicographic_and_median_ties(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_lex_tie() + fc.case_median_tie(), want=(3, 1, 0))


@pytest.mark.parametrize("seed", [400, 403])
def test_noisy_groups_are_repaired_in_the_third_round(oracle, locus, ctxs, seed):
    _, refs, _, _ = _check(oracle, locus, ctxs, fc.case_noisy(seed), want=(1, 1, 0))
    assert refs[0]["stats"]["n_wfa_cons"] > 0


def test_more_than_64_reads(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_100_reads() + fc.case_256_reads(), want=(2, 0, 0))


def test_long_segments(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_long_segments(), want=(1, 1, 0))


def test_purity_filter_on(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_purity(), params=locus.Params(min_read_qual=0.5), want=(3, 0, 0))


def test_random_loci(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_random())


def test_mixed_batch_keeps_the_two_settings_apart(oracle, locus, ctxs):
    from trgt_amd import _lib
    loci = fc.case_mixed()
    params = locus.Params()
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, want=(2, 0, 0))
    # both settings on: trgt_hip_flank_stats counts the size loci only -- [0], [1], [3] by the size route's restatement; [2], device-genotyped
    # loci sent to the host path for the flank step, is the cluster locus whose flank SNVs split it, as on a context without the new setting
    size_stats = _expected_stats(loci, plain, sent=1)
    assert size_stats == (2, 0, 1, 0)
    both = dict(ctxs)["both"]
    for how, out in _runs(locus, b, params, both):
        assert both.flank_stats() == size_stats and both.flank_cluster_stats() == (2, 0, 0), how
    # the 300-read locus on the deep chain: genotyped on the device, redone by the host as before, not this route's
    deep = _lib.Context(0)
    try:
        deep.set_flank_cluster_device(True)
        deep.set_cluster_max_reads(512)
        for how, out in _runs(locus, b, params, deep):
            _compare(locus, b, out, refs, ("deep", how))
            assert deep.flank_cluster_stats() == (2, 0, 0), how
    finally:
        deep.close()


def test_no_room_for_the_third_round_hands_the_locus_back(oracle, locus, ctxs):
    """The arenas are not rolled back between the rounds.  With every segment 54 or 57 bases long, round 1 of the cluster chain (two groups,
    at most 24 members in all) takes at most r1_max whatever the grouping and at least r1_min; round 3 (both tag groups, 12 members each,
    backbones of at least 54) at least r3_min of CIGAR words.  TRGT_CLUSTER_ARENA_KB = kb caps the CIGAR arena at 256 kb words."""
    from trgt_amd import _lib
    lo, hi, n = 54, 57, 24
    r1_max = (n * (hi + 1) + n * hi, n * hi + 2 * (hi + 16 + 15), 3 * n)  # CIGAR words, result bytes, scratch words
    r1_min = 2 * group_needs(lo, 1, lo)[0]
    r3_min = 2 * group_needs(lo, 12, 12 * lo)[0]
    kb = -(-r1_max[0] // 256)
    assert r1_max[0] <= kb * 256 < r1_min + r3_min and r1_max[1] <= kb * 1024 and r1_max[2] <= kb * 256
    loci = fc.case_no_room()
    ctx = _lib.context_with_env(TRGT_CLUSTER_ARENA_KB=kb)
    try:
        ctx.set_flank_cluster_device(True)
        _, _, _, outs = _check(oracle, locus, ctxs, loci, handed=(0,), want=(0, 0, 1), only=ctx)
        for name, how, out in outs:
            assert int(out.stats[22]) == 1 and int(out.stats[23]) == 0, how
    finally:
        ctx.close()


def test_other_entry_points(oracle, locus, ctxs):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = dict(ctxs)["on"]
    loci = fc.case_het() + fc.case_noisy() + fc.case_tags_against_clusters()
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, only=on)
    stats = fc.expected_stats(loci, plain)
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, ctx=on))
    assert recs(b, locus.submit_batch(b, ctx=on).wait()) == want and on.flank_cluster_stats() == stats
    got, total = [], [0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, ctx=on))
        total = [x + y for x, y in zip(total, on.flank_cluster_stats())]
    assert got == want and tuple(total) == stats
    pool = _lib.Pool([0, 0], flank_cluster_device=True)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
    finally:
        pool.close()
    # the setting on a batch without hp_tag: nothing to do, nothing counted
    bare = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    _compare(locus, bare, locus.run_batch(bare, ctx=on, reads_dev=torch.from_numpy(bare["read_blob"]).cuda()), plain, "no hp_tag")
    assert on.flank_cluster_stats() == (0, 0, 0)
