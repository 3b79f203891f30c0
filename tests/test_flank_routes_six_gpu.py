"""The six opt-in device routes of genotype_flank in ONE call: the five of tests/test_flank_routes_combined_gpu.py and the SNV branch
behind the deep cluster chain (trgt_hip_set_snv_cluster_deep_device).  That module stays as it is and pins the five; this one mirrors it
with a batch that holds a locus of every one of the six routes -- its batch plus a 257-read cluster locus split by SNVs -- on a context
with every setting on, with the new setting on alone, and on a context as it is created.

Every output array must equal the all-off run's bit for bit (which is held to the oracle), and each of the seven statistics must be what
the case modules' restatements say (computed from the oracle's plain result, never from the library); a route that is off reports zeros."""
import pytest

import flank_cluster_cases as fcl
import flank_cluster_deep_cases as fcd
import flank_deep_cases as fd
import snv_cluster_deep_cases as scd
import snv_deep_cases as sd
import test_flank_routes_combined_gpu as five
from test_flank_device_gpu import _compare, _ref

pytestmark = pytest.mark.gpu
ZERO3, ZERO4 = five.ZERO3, five.ZERO4
CLUSTER_DEEP_SNV = "snv_cluster_deep_device"
ROUTES = five.ROUTES + (CLUSTER_DEEP_SNV,)


def case_six():
    """(loci, the route that owns each or None): the five-route batch, and behind it the locus of the sixth"""
    import numpy as np
    loci, owner = five.case_combined()
    rng = np.random.default_rng(701)
    return loci + scd.cl([sd.het(rng, five.DEEP_READS)]), owner + [CLUSTER_DEEP_SNV]


def expected(loci, owner, plain, on, size_max, cluster_max):
    want = five.expected(loci, owner, plain, on, size_max, cluster_max)
    want["snv_cluster_deep_stats"] = scd.expected_stats(loci, plain, cluster_max) if CLUSTER_DEEP_SNV in on and cluster_max > fd.SHALLOW else ZERO4
    return want


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def limits():
    from trgt_amd import _lib
    return _lib.size_max_reads_limit(), _lib.cluster_max_reads_limit()


@pytest.fixture(scope="module")
def case(oracle, locus):
    from trgt_amd import _lib
    loci, owner = case_six()
    params = locus.Params(**fd.DEEP)
    b = locus.pack(loci)
    plain = fcl.plain_results(oracle, loci, params)
    ctx = _lib.Context(0)
    try:
        off = locus.run_batch(b, params, ctx=ctx)
        got = {k: getattr(ctx, k)() for k in expected(loci, owner, plain, (), fd.SHALLOW, fd.SHALLOW)}
    finally:
        ctx.close()
    _compare(locus, b, off, [_ref(oracle, L, params) for L in loci], "all off")
    assert all(not any(v) for v in got.values()), got
    return loci, owner, plain, params, b, off


def _run(locus, case, limits, on, depth):
    from trgt_amd import _lib
    loci, owner, plain, params, b, off = case
    size_max, cluster_max = limits if depth else (fd.SHALLOW, fd.SHALLOW)
    want = expected(loci, owner, plain, on, size_max, cluster_max)
    ctx = _lib.Context(0)
    try:
        for name in on:
            getattr(ctx, "set_" + name)(True)
        if depth:
            ctx.set_size_max_reads(size_max); ctx.set_cluster_max_reads(cluster_max)
        out = locus.run_batch(b, params, ctx=ctx)
        got = {k: getattr(ctx, k)() for k in want}
    finally:
        ctx.close()
    print(on, "depth settings" if depth else "no depth settings", got, "expected", want)
    five._same_outputs(b, out, off, (on, depth))
    assert got == want, (on, depth)
    return want


def test_the_batch_holds_a_locus_of_every_route(case):
    """conditions of the case, from the restatements alone: each route settles its own loci and no other, nothing is handed back"""
    loci, owner, plain, _, _, _ = case
    assert sorted(set(o for o in owner if o)) == sorted(ROUTES)
    want = expected(loci, owner, plain, ROUTES, fd.CEILING, fcd.CEILING)
    assert want == dict(flank_stats=(2, 0, 0, 1), snv_split_stats=(2, 0, 0, 0), size_deep_stats=(3, 0, 0, 1), flank_cluster_stats=(1, 0, 0),
                        snv_cluster_stats=(1, 0, 0, 0), flank_cluster_deep_stats=(1, 0, 0), snv_cluster_deep_stats=(1, 0, 0, 0))
    assert five.sent_to_host(loci, owner, ROUTES, fd.CEILING, fcd.CEILING) == set()
    assert five.sent_to_host(loci, owner, five.ROUTES, fd.CEILING, fcd.CEILING) == {len(loci) - 1}  # without the sixth setting the host redoes its locus


def test_statistics_refuse_a_null_out_on_a_live_context():
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    try:
        assert _lib.lib().trgt_hip_snv_cluster_deep_stats(ctx.handle, None) == -1
        assert ctx.snv_cluster_deep_stats() == ZERO4
    finally:
        ctx.close()


def test_all_six_settings_on(locus, case, limits):
    _run(locus, case, limits, ROUTES, True)


@pytest.mark.parametrize("depth", [True, False], ids=["depth settings", "no depth settings"])
def test_the_sixth_setting_alone(locus, case, limits, depth):
    want = _run(locus, case, limits, (CLUSTER_DEEP_SNV,), depth)
    assert all(not any(v) for k, v in want.items() if k not in ("snv_cluster_deep_stats", "size_deep_stats")), want
    assert want["snv_cluster_deep_stats"] == ((1, 0, 0, 0) if depth else ZERO4)


def test_the_five_older_settings_leave_the_sixth_locus_to_the_host(locus, case, limits):
    want = _run(locus, case, limits, five.ROUTES, True)
    assert want["snv_cluster_deep_stats"] == ZERO4
