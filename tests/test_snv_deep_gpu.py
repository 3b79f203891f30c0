"""The SNV branch of genotype_flank (get_trs_with_clustering, genotype_flank.rs:78-138, 171-290; applied at tr.rs:69-75) for
Genotyper::Size loci of 257 to 2 048 candidate reads: the SNV forms of the two deep size kernels (locus_gt_deep.hpp), which run on a
context with trgt_hip_set_snv_split_device and trgt_hip_set_size_max_reads both set, for a batch that carries mismatch offsets.

Every case of snv_deep_cases.py is compared bit for bit with the oracle's restatement of analyze_tr -- alleles, kept reads and their
order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS / AP -- with host reads and with reads resident
in HBM, on six contexts: both settings, both with trgt_hip_set_flank_device as well, size_max_reads alone, the SNV setting alone,
neither, TRGT_HOST_GENOTYPER=1; `flipped`, which the oracle does not report, must agree among them.  trgt_hip_snv_split_stats and
trgt_hip_size_deep_stats must be what the oracle's plain result and the plain-Python restatement of the branch predict
(snv_deep_cases.expected_stats; the conditions of the cases: test_snv_deep_cases.py): with both settings the deep loci are counted and
out[3] of the deep statistics counts those the SNV branch settled; with one setting alone nothing changes -- no deep locus in the SNV
statistics, out[3] = 0."""
import numpy as np
import pytest

import flank_deep_cases as fc
import snv_deep_cases as dc
import snv_split_cases as sc
from test_flank_device_gpu import _compare, _ref, _runs

pytestmark = pytest.mark.gpu
ZERO = (0, 0, 0, 0)
ON = ("both", "both + flank")


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
    both, three, size, snv, neither, host = [_lib.Context(0) for _ in range(5)] + [_lib.context_with_env(TRGT_HOST_GENOTYPER=1)]
    both.set_snv_split_device(True); both.set_size_max_reads(limit)
    three.set_snv_split_device(True); three.set_size_max_reads(limit); three.set_flank_device(True)
    size.set_size_max_reads(limit)
    snv.set_snv_split_device(True)
    yield [("both", both), ("both + flank", three), ("size only", size), ("snv only", snv), ("neither", neither), ("host genotyper", host)]
    for c in (both, three, size, snv, neither, host):
        c.close()


def _expect(loci, plain, max_reads, handed):
    """per context name: (snv_split_stats, size_deep_stats, (flank_stats[0], [1], [3]))"""
    return {"both": dc.expected_stats(loci, plain, max_reads, handed) + ((0, 0, 0),),
            "both + flank": dc.expected_stats(loci, plain, max_reads, handed, flank_device=True) + (dc.tag_route_stats(loci, plain, max_reads, handed),),
            "size only": (ZERO, fc.size_only_stats(loci, plain, max_reads), (0, 0, 0)),
            "snv only": (sc.expected_stats(loci, plain, handed), ZERO, (0, 0, 0)),
            "neither": (ZERO, ZERO, (0, 0, 0))}


def _check(oracle, locus, ctxs, loci, kw=dc.DEEP, handed=(), want=None, on_ctxs=None, max_reads=dc.CEILING):
    """want: what the case itself expects of the two statistics with both settings on (checked against the restatement before any GPU
    run).  on_ctxs: contexts of the case's own, (name, context) with the names of the module's."""
    params = locus.Params(**kw)
    b = locus.pack(loci)
    refs, plain = fc.oracle_pair(oracle, loci, params)
    expect = _expect(loci, plain, max_reads, handed)
    if want is not None:
        assert expect["both"][:2] == want
    flipped = []
    for name, ctx in (on_ctxs if on_ctxs is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            if name in expect:
                got = (ctx.snv_split_stats(), ctx.size_deep_stats(), ctx.flank_stats())
                print(name, how, "snv_split_stats, size_deep_stats, flank_stats", got, "expected", expect[name])
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            if name in expect:
                assert got[:2] == expect[name][:2], (name, how)
                assert (got[2][0], got[2][1], got[2][3]) == expect[name][2], (name, how)
                if name not in ON:
                    assert got[1][3] == 0, (name, how)
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, expect["both"][:2]


def test_depths_and_rounds(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, dc.case_depths(), want=((4, 0, 0, 0), (2, 0, 0, 2)))


@pytest.mark.parametrize("n", sorted(dc.SKIPS))
def test_skip_rounding_and_rank_selection(oracle, locus, ctxs, n):
    _check(oracle, locus, ctxs, dc.case_skip(n)[0], want=((2, 0, 0, 0), (4, 0, 0, 2)))


def test_call_threshold_and_fewest_fully_observed_reads(oracle, locus, ctxs):
    assert 52.0 / 260.0 >= 0.20 and not 51.0 / 260.0 >= 0.20
    _check(oracle, locus, ctxs, dc.case_call_threshold() + dc.case_least_full(), want=((2, 0, 0, 0), (3, 0, 0, 2)))


def test_ties_alternate_across_the_rounds_and_join_both_groups(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, dc.case_ties(), want=((1, 1, 0, 0), (1, 1, 0, 1)))
    assert refs[0]["stats"]["n_wfa_cons"] > 0


def test_undecided_searches_and_a_decided_one(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, dc.case_margin(), want=((1, 0, 0, 2), (1, 0, 2, 1)))


def test_repair_swap_and_reference_first(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, dc.case_repair(), want=((4, 2, 0, 0), (4, 2, 0, 4)))
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs[:2])
    assert refs[2]["alleles"] == [dc.CAG20.decode(), dc.CAG21.decode()] and refs[3]["alleles"] == [dc.CAG21.decode(), dc.CAG20.decode()]


@pytest.mark.parametrize("env", [dict(TRGT_REPAIR_MAX_SEG=60), dict(TRGT_HOST_REPAIR=1)])
def test_handing_back(oracle, locus, ctxs, limit, env):
    from trgt_amd import _lib
    ctx = _lib.context_with_env(**env)
    try:
        ctx.set_snv_split_device(True); ctx.set_size_max_reads(limit)
        _check(oracle, locus, ctxs, dc.case_hand_back(), handed=(0,), want=((1, 0, 1, 0), (1, 0, 1, 1)), on_ctxs=[("both", ctx)])
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["snv", "hap", "offset"])
def test_limits(oracle, locus, ctxs, case):
    loci = {"snv": dc.case_snv_cap, "hap": dc.case_hap_cap, "offset": dc.case_offset_cap}[case]()
    _check(oracle, locus, ctxs, loci, want=((1, 0, 1, 0), (1, 0, 1, 1)))  # at the cap: settled; one beyond: handed back


def test_tags_and_snvs_together(oracle, locus, ctxs):
    # the tags of [0] split: the tag route's where the flank setting is on as well, the host's otherwise (counted [0] by the deep
    # statistics either way: the device genotyped it); [1] and [2] are the SNV route's
    _check(oracle, locus, ctxs, dc.case_tags_and_snvs(), want=((2, 0, 0, 0), (3, 0, 0, 2)))


def test_mixed_batch_and_a_locus_beyond_the_setting(oracle, locus, ctxs):
    from trgt_amd import _lib
    loci = dc.case_mixed()
    _check(oracle, locus, ctxs, loci, want=((4, 0, 0, 0), (5, 0, 0, 3)))
    own = [("both", _lib.Context(0)), ("both + flank", _lib.Context(0))]
    try:
        for _, c in own:
            c.set_snv_split_device(True); c.set_size_max_reads(dc.MIXED_SETTING)
        own[1][1].set_flank_device(True)
        # the 301-read locus is the host's from the start: neither statistic counts it
        _check(oracle, locus, ctxs, loci, want=((3, 0, 0, 0), (4, 0, 0, 2)), on_ctxs=own, max_reads=dc.MIXED_SETTING)
    finally:
        for _, c in own:
            c.close()


def test_purity_filter_on(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, dc.case_purity(), dict(dc.PURITY, **dc.DEEP), want=((2, 0, 0, 0), (2, 0, 0, 2)))


def test_random_loci(oracle, locus, ctxs):
    _, _, (snv, deep) = _check(oracle, locus, ctxs, dc.case_random())
    assert snv[0] >= 10 and snv[1] >= 3 and deep[3] == snv[0]


def test_other_entry_points(oracle, locus, ctxs, limit):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = ctxs[0][1]
    loci = dc.case_depths() + dc.case_repair()[:2] + dc.case_margin()[:1]
    params = locus.Params(**dc.DEEP)
    b, refs, (stats, deep_stats) = _check(oracle, locus, ctxs, loci, on_ctxs=[("both", on)], want=((6, 2, 0, 1), (4, 2, 1, 4)))
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, params, ctx=on))
    assert recs(b, locus.submit_batch(b, params, ctx=on).wait()) == want and on.snv_split_stats() == stats and on.size_deep_stats() == deep_stats
    got, total, dtotal = [], [0, 0, 0, 0], [0, 0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, params, ctx=on))
        total = [x + y for x, y in zip(total, on.snv_split_stats())]
        dtotal = [x + y for x, y in zip(dtotal, on.size_deep_stats())]
    assert got == want and tuple(total) == stats and tuple(dtotal) == deep_stats
    pool = _lib.Pool([0, 0], snv_split_device=True, size_max_reads=limit)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks, params)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
        assert sum(c.size_deep_stats()[3] for c in pool.contexts) > 0
    finally:
        pool.close()
    # both settings on a batch without mismatch arrays: the length genotype on the device, nothing counted for the route
    plain = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    ref_plain = [_ref(oracle, L, params, meta=False) for L in loci]
    _compare(locus, plain, locus.run_batch(plain, params, ctx=on, reads_dev=torch.from_numpy(plain["read_blob"]).cuda()), ref_plain, "no mismatch arrays")
    assert on.snv_split_stats() == ZERO and on.size_deep_stats() == fc.size_only_stats(loci, ref_plain, limit)
