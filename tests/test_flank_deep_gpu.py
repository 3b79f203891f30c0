"""The haplotype-tag branch of genotype_flank (get_trs_with_hp, genotype_flank.rs:43-76, simple_consensus :147-170; applied at tr.rs:69-75)
for Genotyper::Size loci of 257 to 2 048 candidate reads: the FLANK forms of the two deep size kernels (locus_gt_deep.hpp), which run on a
context with trgt_hip_set_flank_device and trgt_hip_set_size_max_reads both set.

Every case compares alleles, kept reads and their order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS /
AP with the oracle's restatement of analyze_tr, with host reads and with reads resident in HBM, on five contexts: both settings, the flank
setting alone, size_max_reads alone, neither, TRGT_HOST_GENOTYPER=1; `flipped`, which the oracle does not report, must agree among the
five.  What trgt_hip_flank_stats and trgt_hip_size_deep_stats must report is computed from the oracle's plain result (no read metadata)
and a restatement of the tag rule (flank_deep_cases.py), never taken from the library: with both settings the deep loci are counted, and
out[3] of the flank statistics counts them; with the flank setting alone they are the host's from the start.  The conditions the cases
claim are checked without a GPU in test_flank_deep_cases.py."""
import numpy as np
import pytest

import flank_deep_cases as fc
from test_flank_device_gpu import _compare, _runs

pytestmark = pytest.mark.gpu
ZERO = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def limit():
    from trgt_amd import _lib
    return _lib.size_max_reads_limit()


@pytest.fixture(scope="module")
def ctxs(limit):
    from trgt_amd import _lib
    both, flank, size, neither, host = _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.context_with_env(TRGT_HOST_GENOTYPER=1)
    both.set_flank_device(True); both.set_size_max_reads(limit)
    flank.set_flank_device(True)
    size.set_size_max_reads(limit)
    yield [("both", both), ("flank only", flank), ("size only", size), ("neither", neither), ("host genotyper", host)]
    for c in (both, flank, size, neither, host):
        c.close()


def _check(oracle, locus, ctxs, loci, kw=None, sent=(), handed=(), want=None, both_ctx=None, max_reads=fc.CEILING):
    """want: what the case itself expects of the two statistics with both settings on (checked against the restatement before any GPU
    run).  both_ctx: a context of the case's own with both settings, run alone."""
    params = locus.Params(**(kw or {}))
    b = locus.pack(loci)
    refs, plain = fc.oracle_pair(oracle, loci, params)
    expect = {"both": fc.expected_stats(loci, plain, max_reads, sent, handed),
              "flank only": (fc.expected_stats(loci, plain, fc.SHALLOW, sent, handed)[0], ZERO),
              "size only": (ZERO, fc.size_only_stats(loci, plain, max_reads)), "neither": (ZERO, ZERO)}
    if want is not None:
        assert expect["both"] == want
    flipped = []
    for name, ctx in ([("both", both_ctx)] if both_ctx is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            if name in expect:
                got = (ctx.flank_stats(), ctx.size_deep_stats())
                print(name, how, "flank_stats, size_deep_stats", got, "expected", expect[name])
                assert got == expect[name], (name, how)
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, expect["both"]


def test_depths_and_rounds(oracle, locus, ctxs):
    (one, kw1), (many, kw2) = fc.case_depths()
    _check(oracle, locus, ctxs, one, kw1, want=((1, 0, 0, 1), (1, 0, 0, 0)))
    _check(oracle, locus, ctxs, many, kw2, want=((5, 0, 0, 3), (3, 0, 0, 0)))


def test_the_ceiling(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, fc.case_ceiling(), fc.DEEP, want=((1, 0, 0, 1), (1, 0, 0, 0)))


@pytest.mark.parametrize("kw", [{}, fc.DEEP])
def test_tags_against_lengths(oracle, locus, ctxs, kw):
    _check(oracle, locus, ctxs, fc.case_tags_against_lengths(), kw, want=((1, 0, 0, 1), (1, 0, 0, 0)))


def test_acceptance_threshold(oracle, locus, ctxs):
    assert 182.0 / 260.0 >= 0.7 and not 181.0 / 260.0 >= 0.7
    _check(oracle, locus, ctxs, fc.case_threshold(), fc.DEEP, want=((2, 0, 0, 2), (5, 0, 0, 0)))  # refused loci carry no mismatches: they stay on the device


def test_untagged_reads_alternate_across_the_rounds(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, fc.case_boundary(), fc.DEEP, want=((1, 0, 0, 1), (1, 0, 0, 0)))
    assert refs[0]["alleles"] == [fc.X60.decode(), fc.W63.decode()]


def test_consensus_ties(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, fc.case_ties(), fc.DEEP, want=((3, 1, 0, 3), (3, 1, 0, 0)))
    assert all(fc.CAG20.decode() in r["alleles"] for r in refs)


def test_repair_one_group_both_groups_and_swap(oracle, locus, ctxs):
    loci = fc.case_repair()
    _, refs, _ = _check(oracle, locus, ctxs, loci, fc.DEEP, want=((3, 3, 0, 3), (3, 3, 0, 0)))
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs)
    sw = refs[2]
    assert [int(v) for v in sw["classification"]] == [1 - (loci[2]["hp_tag"][int(r)] - 1) for r in sw["kept_read"]]


def test_repair_at_the_ceiling(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, fc.case_ceiling(noisy=True), fc.DEEP, want=((1, 1, 0, 1), (1, 1, 0, 0)))
    assert refs[0]["stats"]["n_wfa_cons"] > 0


def test_reference_allele_first_after_the_swap(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, fc.case_reference_first(), fc.DEEP, want=((2, 0, 0, 2), (2, 0, 0, 0)))
    assert refs[0]["alleles"] == [fc.CAG20.decode(), fc.CAG21.decode()] and refs[1]["alleles"] == [fc.CAG21.decode(), fc.CAG20.decode()]


@pytest.mark.parametrize("kw", [fc.PURITY, dict(fc.PURITY, **fc.DEEP)])
def test_purity_filter_on(oracle, locus, ctxs, kw):
    _check(oracle, locus, ctxs, fc.case_purity(), kw, want=((2, 0, 0, 2), (2, 0, 0, 0)))


@pytest.mark.parametrize("env", [dict(TRGT_REPAIR_MAX_SEG=60), dict(TRGT_HOST_REPAIR=1)])
def test_handing_back(oracle, locus, ctxs, limit, env):
    from trgt_amd import _lib
    ctx = _lib.context_with_env(**env)
    try:
        ctx.set_flank_device(True); ctx.set_size_max_reads(limit)
        _check(oracle, locus, ctxs, fc.case_hand_back(), fc.DEEP, handed=(0,), want=((1, 0, 1, 1), (1, 0, 1, 0)), both_ctx=ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("kw", [{}, fc.DEEP])
def test_mixed_call(oracle, locus, ctxs, limit, kw):
    loci, snv = fc.case_mixed(limit)
    _check(oracle, locus, ctxs, loci, kw, sent=snv, want=((3, 0, 2, 2), (5, 0, 0, 0)))


def test_a_setting_below_the_ceiling(oracle, locus, ctxs):
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    try:
        ctx.set_flank_device(True); ctx.set_size_max_reads(300)
        _check(oracle, locus, ctxs, fc.case_setting_300(), fc.DEEP, want=((1, 0, 0, 1), (1, 0, 0, 0)), both_ctx=ctx, max_reads=300)  # the 301-read locus is the host's
    finally:
        ctx.close()


def test_other_entry_points(oracle, locus, ctxs, limit):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    from test_flank_device_gpu import _ref
    on = ctxs[0][1]
    loci = fc.case_entry_points()
    params = locus.Params(**fc.DEEP)
    b, refs, (stats, deep_stats) = _check(oracle, locus, ctxs, loci, fc.DEEP, both_ctx=on, want=((5, 1, 0, 4), (4, 1, 0, 0)))
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, params, ctx=on))
    assert recs(b, locus.submit_batch(b, params, ctx=on).wait()) == want and on.flank_stats() == stats and on.size_deep_stats() == deep_stats
    pk = locus.pack_bam4(b)
    assert recs(pk, locus.run_batch(pk, params, ctx=on)) == want and on.flank_stats() == stats
    got, total, dtotal = [], [0, 0, 0, 0], [0, 0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, params, ctx=on))
        total = [x + y for x, y in zip(total, on.flank_stats())]
        dtotal = [x + y for x, y in zip(dtotal, on.size_deep_stats())]
    assert got == want and tuple(total) == stats and tuple(dtotal) == deep_stats
    pool = _lib.Pool([0, 0], flank_device=True, size_max_reads=limit)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks, params)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
    finally:
        pool.close()
    # both settings on a batch without hp_tag: the length genotype on the device, nothing counted for the route
    plain = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    ref_plain = [_ref(oracle, L, params, meta=False) for L in loci]
    _compare(locus, plain, locus.run_batch(plain, params, ctx=on, reads_dev=torch.from_numpy(plain["read_blob"]).cuda()), ref_plain, "no hp_tag")
    assert on.flank_stats() == ZERO and on.size_deep_stats() == fc.size_only_stats(loci, ref_plain, limit)


def test_random_loci(oracle, locus, ctxs):
    """Conditions, not measurements (asserted without a GPU in test_flank_deep_cases.py too): by the restatement at least 5 of the 12 loci
    go down the route and at least 2 of those are repaired.  out[2] depends on the SNV branch, which has no few-line restatement: bounded,
    not pinned."""
    routed = repaired = 0
    for loci, kw in fc.case_random():
        params = locus.Params(**kw)
        b = locus.pack(loci)
        refs, plain = fc.oracle_pair(oracle, loci, params)
        stats, deep_stats = fc.expected_stats(loci, plain, fc.CEILING)
        routed += stats[0]; repaired += stats[1]
        for name, ctx in ctxs:
            for how, out in _runs(locus, b, params, ctx):
                _compare(locus, b, out, refs, (name, how))
                if name == "both":
                    got = ctx.flank_stats()
                    print("random", how, got, ctx.size_deep_stats(), "expected", stats, deep_stats)
                    assert (got[0], got[1], got[3]) == (stats[0], stats[1], stats[3]) and 0 <= got[2] <= len(loci) - got[0]
                    assert ctx.size_deep_stats() == deep_stats
                elif name in ("flank only", "neither"):
                    assert ctx.flank_stats() == ZERO and ctx.size_deep_stats() == ZERO
                elif name == "size only":
                    assert ctx.flank_stats() == ZERO and ctx.size_deep_stats() == fc.size_only_stats(loci, plain, fc.CEILING)
    assert routed >= 5 and repaired >= 2
