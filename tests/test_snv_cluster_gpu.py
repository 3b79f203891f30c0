"""The SNV branch of genotype_flank (get_trs_with_clustering, genotype_flank.rs:78-138, 171-290; applied by analyze at tr.rs:64-75
whichever genotyper produced the alleles) behind the one-wave cluster chain: the SNV forms of trgt_amd/csrc/locus_cluster_flank.hpp,
opt-in per context through trgt_hip_set_snv_cluster_device.

Every case compares alleles, kept reads and their order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS /
AP with the oracle's restatement of analyze_tr, for five contexts -- the setting on, the setting together with
trgt_hip_set_flank_cluster_device, the tag setting only, a context as it is created, TRGT_HOST_CLUSTER=1 with the setting on -- and with
the reads on the host and resident in HBM; `flipped`, which the oracle does not report, must agree between them.  The results are the
host redo's on every context: what fails without the route are the statistics, which tests/snv_cluster_cases.py computes from the
oracle's plain result and the plain-Python restatement of the branch (asserted before any GPU run).  The conditions of the cases
themselves are asserted without a GPU in tests/test_snv_cluster_cases.py."""
import numpy as np
import pytest

import flank_cluster_cases as fc
import snv_cluster_cases as cc
import snv_split_cases as sc
from test_flank_device_gpu import _compare, _ref, _runs
from test_repair_needs import group_needs

pytestmark = pytest.mark.gpu
ZERO = (0, 0, 0, 0)
SNV_ON = ("snv", "both")


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def ctxs():
    from trgt_amd import _lib
    snv, both, tags, off, host = _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.context_with_env(TRGT_HOST_CLUSTER=1)
    snv.set_snv_cluster_device(True)
    both.set_snv_cluster_device(True)
    both.set_flank_cluster_device(True)
    tags.set_flank_cluster_device(True)
    host.set_snv_cluster_device(True)  # (no device cluster chain: the setting has nothing to follow)
    yield [("snv", snv), ("both", both), ("tags", tags), ("off", off), ("host cluster", host)]
    for c in (snv, both, tags, off, host):
        c.close()


def _check(oracle, locus, ctxs, loci, params=None, handed=(), want=None, tag_want=None, only=None):
    """want: what the case itself expects of trgt_hip_snv_cluster_stats (checked against the restatement before any GPU run); tag_want: of
    trgt_hip_flank_cluster_stats per context name (default: zeros); only: one context (which has the setting on) instead of the five"""
    params = params or locus.Params()
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = [_ref(oracle, L, params, meta=False) for L in loci]
    stats = cc.expected_stats(loci, plain, handed)
    if want is not None:
        assert stats == want
    flipped, outs = [], []
    for name, ctx in ([("snv", only)] if only is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            expect = stats if name in SNV_ON else ZERO
            print(name, how, "snv_cluster_stats", ctx.snv_cluster_stats(), "expected", expect, "flank_cluster_stats", ctx.flank_cluster_stats())
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            assert ctx.snv_cluster_stats() == expect, (name, how)
            if tag_want is not None:
                assert ctx.flank_cluster_stats() == tag_want.get(name, (0, 0, 0)), (name, how)
            assert ctx.snv_split_stats() == ZERO and ctx.flank_stats() == ZERO, (name, how)
            outs.append((name, how, out))
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, plain, outs


def test_reference_vectors(oracle, locus, ctxs):
    _, refs, _, _ = _check(oracle, locus, ctxs, cc.case_kats(), want=(1, 0, 0, 0), tag_want={})
    assert [int(v) for v in refs[0]["classification"]] == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("n", [3, 10, 30])
def test_sites_at_the_edges_of_the_region(oracle, locus, ctxs, n):
    _check(oracle, locus, ctxs, cc.case_skip(n)[0], want=(2, 0, 0, 0))


def test_call_threshold_and_fewest_fully_observed_reads(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, cc.case_call_threshold() + cc.case_least_full(), want=(2, 0, 0, 0))


def test_overlapping_groups(oracle, locus, ctxs):
    """num_spanning follows the assignment (5 / 5), consensus and intervals the membership (6 members each)"""
    _, refs, _, outs = _check(oracle, locus, ctxs, cc.case_ties(), want=(1, 0, 0, 0))
    assert sc.Y60.decode() in refs[0]["alleles"]
    assert sorted(tuple(int(v) for v in c) for c in refs[0]["gt_ci"]) == [(60, 66), (60, 66)]
    for name, how, out in outs:
        assert [int(v) for v in out.num_spanning[:2]] == [5, 5], (name, how)


def test_last_maximum_and_margin(oracle, locus, ctxs):
    loci = cc.case_margin()
    _check(oracle, locus, ctxs, loci[:2], want=(0, 0, 0, 2), tag_want={})
    _check(oracle, locus, ctxs, loci, want=(1, 0, 0, 2))


def test_repair_swap_and_reference_first(oracle, locus, ctxs):
    _, refs, _, _ = _check(oracle, locus, ctxs, cc.case_repair(), want=(4, 2, 0, 0), tag_want={})
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs[:2])


def test_no_room_for_the_third_round_hands_the_locus_back(oracle, locus, ctxs):
    """As tests/test_flank_cluster_gpu.py makes it: the arenas are not rolled back between the rounds.  With every segment 54 or 57 bases
    long, round 1 of the cluster chain (two groups, at most 24 members in all) takes at most r1_max whatever the grouping and at least
    r1_min; round 3 (both SNV groups, 12 members each, no read in both, backbones of at least 54) at least r3_min of CIGAR words.
    TRGT_CLUSTER_ARENA_KB = kb caps the CIGAR arena at 256 kb words."""
    from trgt_amd import _lib
    lo, hi, n = 54, 57, 24
    r1_max = (n * (hi + 1) + n * hi, n * hi + 2 * (hi + 16 + 15), 3 * n)  # CIGAR words, result bytes, scratch words
    r1_min = 2 * group_needs(lo, 1, lo)[0]
    r3_min = 2 * group_needs(lo, 12, 12 * lo)[0]
    kb = -(-r1_max[0] // 256)
    assert r1_max[0] <= kb * 256 < r1_min + r3_min and r1_max[1] <= kb * 1024 and r1_max[2] <= kb * 256
    ctx = _lib.context_with_env(TRGT_CLUSTER_ARENA_KB=kb)
    try:
        ctx.set_snv_cluster_device(True)
        _check(oracle, locus, ctxs, cc.case_no_room(), handed=(0,), want=(0, 0, 1, 0), tag_want={}, only=ctx)
    finally:
        ctx.close()


def test_an_allele_beyond_allele_cap_is_the_hosts_error(oracle, locus, ctxs):
    """the chain's own alleles (60 / 60) fit the buffer, the SNV split's (63) does not: the route hands the locus back, and the host path
    reports the error as it does without the setting"""
    from trgt_amd import _lib
    loci = cc.case_allele_cap()
    params = locus.Params()
    plain = [_ref(oracle, L, params, meta=False) for L in loci]
    assert cc.expected_stats(loci, plain, handed=(0,)) == (0, 0, 1, 0)
    b = locus.pack(loci)
    for name, ctx in ctxs:
        small = locus.BatchOutputs(b)
        small.allele_cap[:] = cc.ALLELE_CAP
        with pytest.raises(_lib.TrgtHipError, match="allele_cap"):
            locus.run_batch(b, params, ctx, outputs=small)
        assert ctx.snv_cluster_stats() == ((0, 0, 1, 0) if name in SNV_ON else ZERO), name
        _compare(locus, b, locus.run_batch(b, params, ctx), [_ref(oracle, L, params) for L in loci], (name, "the context is still usable"))


def test_large_instantiation(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, cc.case_forms(), want=(3, 0, 0, 0))


@pytest.mark.parametrize("n,big", [(20, False), (40, True)])
def test_segments_of_501_and_504_bases(oracle, locus, ctxs, n, big):
    _check(oracle, locus, ctxs, cc.case_segments_beyond_lds(n, big), want=(2 if big else 1, 0, 0, 0))


def test_purity_filter_on(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, cc.case_purity(), params=locus.Params(min_read_qual=0.5), want=(3, 0, 0, 0))


@pytest.mark.parametrize("case", ["snv", "hap", "offset small", "offset big"])
def test_limits(oracle, locus, ctxs, case):
    loci = {"snv": cc.case_snv_cap, "hap": cc.case_hap_cap, "offset small": lambda: cc.case_offset_cap(False), "offset big": lambda: cc.case_offset_cap(True)}[case]()
    _check(oracle, locus, ctxs, loci, want=(1, 0, 1, 0), tag_want={})  # at the cap: settled; one beyond: handed back


def test_tags_and_snvs_together(oracle, locus, ctxs):
    # the tags of [0] split: the tag branch where its setting is on (alone or with this one), the host where this one is alone (no count
    # anywhere); [1] is the SNV branch's wherever this setting is on
    _check(oracle, locus, ctxs, cc.case_tags_and_snvs(), want=(1, 0, 0, 0), tag_want={"both": (1, 0, 0), "tags": (1, 0, 0)})


def test_tag_and_snv_loci_share_the_third_round(oracle, locus, ctxs):
    loci = cc.case_tags_and_snvs_repaired()
    params = locus.Params()
    plain = [_ref(oracle, L, params, meta=False) for L in loci]
    assert fc.expected_stats(loci, plain) == (1, 1, 0)
    # on "both" either locus is settled behind the one third round of the call (one part of the job and group lists, one launch)
    _check(oracle, locus, ctxs, loci, want=(1, 1, 0, 0), tag_want={"both": (1, 1, 0), "tags": (1, 1, 0)})


def test_mixed_batch_keeps_the_two_snv_settings_apart(oracle, locus, ctxs):
    from trgt_amd import _lib
    loci = cc.case_mixed()
    params = locus.Params()
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, want=(1, 0, 0, 0), tag_want={})
    size_stats = sc.expected_stats(loci, plain)
    assert size_stats == (2, 0, 0, 0)
    ctx = _lib.Context(0)
    try:  # the 300-read cluster locus on the deep chain: genotyped on the device, the flank step is the host's; the size loci on their own route
        ctx.set_snv_cluster_device(True)
        ctx.set_snv_split_device(True)
        ctx.set_cluster_max_reads(512)
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, ("all three", how))
            assert ctx.snv_cluster_stats() == (1, 0, 0, 0) and ctx.snv_split_stats() == size_stats and ctx.flank_cluster_stats() == (0, 0, 0), how
    finally:
        ctx.close()


def test_random_loci(oracle, locus, ctxs):
    loci = cc.case_random()
    params = locus.Params()
    plain = [_ref(oracle, L, params, meta=False) for L in loci]
    stats = cc.expected_stats(loci, plain)
    assert stats[3] == 0 and stats[2] == 0 and stats[0] >= 5  # a route that hands everything back undecided cannot pass
    _check(oracle, locus, ctxs, loci, want=stats)


def test_other_entry_points(oracle, locus, ctxs):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = dict(ctxs)["snv"]
    loci = cc.case_kats() + cc.case_repair() + cc.case_margin()
    b, refs, plain, _ = _check(oracle, locus, ctxs, loci, want=(6, 2, 0, 2), only=on)
    stats = (6, 2, 0, 2)
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, ctx=on))
    assert recs(b, locus.submit_batch(b, ctx=on).wait()) == want and on.snv_cluster_stats() == stats
    got, total = [], [0, 0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, ctx=on))
        total = [x + y for x, y in zip(total, on.snv_cluster_stats())]
    assert got == want and tuple(total) == stats
    pool = _lib.Pool([0, 0], snv_cluster_device=True)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
        assert tuple(sum(c.snv_cluster_stats()[k] for c in pool.contexts) for k in range(4))[0] > 0
    finally:
        pool.close()
    # the setting on a batch without mismatch arrays: nothing to do, nothing counted
    bare = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    _compare(locus, bare, locus.run_batch(bare, ctx=on, reads_dev=torch.from_numpy(bare["read_blob"]).cuda()), plain, "no mismatch arrays")
    assert on.snv_cluster_stats() == ZERO
