"""The five opt-in device routes of genotype_flank in ONE call: the tag and SNV branches in the size genotypers (trgt_hip_set_flank_device,
trgt_hip_set_snv_split_device), the tag and SNV branches behind the one-wave cluster chain (trgt_hip_set_flank_cluster_device,
trgt_hip_set_snv_cluster_device) and the tag branch behind the deep cluster chain (trgt_hip_set_flank_cluster_deep_device).  The tests of
the single routes pin each of them with its own batches; this one pins what the host side that drives them decides when a batch holds a
locus of every route at once and carries both hp_tag and mismatch offsets.

The batch: seven loci each built by the module of the route that owns it (a shallow and a 257-read size locus split by tags, a shallow
and a 257-read size locus split by SNVs, a shallow cluster locus split by tags, one split by SNVs, a 257-read cluster locus split by
tags), and one locus of each kind -- size / cluster, shallow / 257 reads -- whose alleles are 30 bases apart, which no route owns.  It runs

  * with the five settings, set_size_max_reads and set_cluster_max_reads on,
  * with each setting on alone, with and without the two depth settings (without them the 257-read loci are the host's from the start),
  * on a context as it is created.

Every output array must equal the last run's bit for bit (which is held to the oracle), and each of the six statistics must be what the
case modules' restatements say for the loci of the batch (computed from the oracle's plain result, never from the library); a route that is
off reports zeros.

trgt_hip_flank_stats[2] also counts the loci the host re-genotypes after the device genotyped them: here every locus that a route owns
splits its reads, so these are the owned loci whose route is off and which the device genotypers took (a 257-read locus only with the depth
setting of its genotyper)."""
import numpy as np
import pytest

import flank_cluster_cases as fcl
import flank_cluster_deep_cases as fcd
import flank_deep_cases as fd
import snv_cluster_cases as scl
import snv_deep_cases as sd
import snv_split_cases as sc
from test_flank_device_gpu import _compare, _ref

pytestmark = pytest.mark.gpu
ZERO3, ZERO4 = (0, 0, 0), (0, 0, 0, 0)
ROUTES = ("flank_device", "snv_split_device", "flank_cluster_device", "snv_cluster_device", "flank_cluster_deep_device")
SIZE_TAG, SIZE_SNV, CLUSTER_TAG, CLUSTER_SNV, CLUSTER_DEEP_TAG = ROUTES
DEEP_READS = 257
CAG30 = b"CAG" * 30
ARRAYS = ("span_start", "span_end", "n_alleles", "allele_len", "ci", "num_spanning", "classification", "read_rank", "n_spans", "motif_counts",
          "gt_size", "flipped")


def case_combined():
    """(loci, the route that owns each or None)"""
    rng = np.random.default_rng(601)
    loci = [(fd._het(rng, 12), SIZE_TAG), (fd._het(rng, DEEP_READS), SIZE_TAG),
            (sc.het(rng, 12), SIZE_SNV), (sd.het(rng, DEEP_READS), SIZE_SNV),
            (fcl._het(rng, 12), CLUSTER_TAG), (scl.cl([sc.het(rng, 12)])[0], CLUSTER_SNV),
            (fcd._het(rng, DEEP_READS), CLUSTER_DEEP_TAG),
            (fd._het(rng, 12, b=CAG30), None), (fd._het(rng, DEEP_READS, b=CAG30), None),
            (fcl._het(rng, 12, b=CAG30), None), (fcd._het(rng, DEEP_READS, b=CAG30), None)]
    return [L for L, _ in loci], [o for _, o in loci]


def sent_to_host(loci, owner, on, size_max, cluster_max):
    """the loci a route owns that the device genotyped and left to the host: the route is off"""
    taken = lambda L: len(L["reads"]) <= (cluster_max if L["genotyper"] == "cluster" else size_max)
    return {l for l, (L, o) in enumerate(zip(loci, owner)) if o is not None and o not in on and taken(L)}


def expected(loci, owner, plain, on, size_max, cluster_max):
    """the six statistics after a call with the settings `on` and the two depth settings (256: not set)"""
    flank = fd.expected_stats(loci, plain, size_max, sent_to_host(loci, owner, on, size_max, cluster_max))
    snv = sd.expected_stats(loci, plain, size_max, flank_device=SIZE_TAG in on)
    deep = ZERO4 if size_max == fd.SHALLOW else snv[1] if SIZE_SNV in on else flank[1] if SIZE_TAG in on else fd.size_only_stats(loci, plain, size_max)
    return dict(flank_stats=flank[0] if SIZE_TAG in on else ZERO4, snv_split_stats=snv[0] if SIZE_SNV in on else ZERO4, size_deep_stats=deep,
                flank_cluster_stats=fcl.expected_stats(loci, plain) if CLUSTER_TAG in on else ZERO3,
                snv_cluster_stats=scl.expected_stats(loci, plain) if CLUSTER_SNV in on else ZERO4,
                flank_cluster_deep_stats=fcd.expected_stats(loci, plain, cluster_max) if CLUSTER_DEEP_TAG in on else ZERO3)


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
    """the batch, its owners, the oracle's plain results, and the outputs of a context as it is created (held to the oracle)"""
    from trgt_amd import _lib
    loci, owner = case_combined()
    params = locus.Params(**fd.DEEP)
    b = locus.pack(loci)
    assert b.get("hp_tag") is not None and b.get("mismatch_offsets") is not None and int(b["mismatch_off"][-1]) > 0
    plain = fcl.plain_results(oracle, loci, params)
    ctx = _lib.Context(0)
    try:
        off = locus.run_batch(b, params, ctx=ctx)
        got = {k: getattr(ctx, k)() for k in expected(loci, owner, plain, (), fd.SHALLOW, fd.SHALLOW)}
    finally:
        ctx.close()
    _compare(locus, b, off, [_ref(oracle, L, params) for L in loci], "all off")
    assert all(v == (ZERO3 if len(v) == 3 else ZERO4) for v in got.values()), got
    return loci, owner, plain, params, b, off


def _same_outputs(b, out, off, how):
    for k in ARRAYS:
        assert np.array_equal(getattr(out, k), getattr(off, k)), (how, k)
    assert out.purity.tobytes() == off.purity.tobytes() or np.array_equal(out.purity, off.purity, equal_nan=True), how
    for s in range(2 * int(b["n_loci"])):  # (the bytes behind an allele and the spans behind n_spans are nobody's)
        o, n = int(off.allele_off[s]), int(off.allele_len[s])
        assert np.array_equal(out.allele_blob[o:o + n], off.allele_blob[o:o + n]), (how, "allele_blob", s)
        o, n = 3 * int(off.span_off[s]), 3 * int(off.n_spans[s])
        assert np.array_equal(out.spans3[o:o + n], off.spans3[o:o + n]), (how, "spans3", s)


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
    _same_outputs(b, out, off, (on, depth))
    assert got == want, (on, depth)
    return want


def test_the_batch_holds_a_locus_of_every_route(case):
    """conditions of the case, from the restatements alone: each route settles its own loci and no other, nothing is handed back"""
    loci, owner, plain, _, _, _ = case
    want = expected(loci, owner, plain, ROUTES, fd.CEILING, fcd.CEILING)
    assert want == dict(flank_stats=(2, 0, 0, 1), snv_split_stats=(2, 0, 0, 0), size_deep_stats=(3, 0, 0, 1), flank_cluster_stats=(1, 0, 0),
                        snv_cluster_stats=(1, 0, 0, 0), flank_cluster_deep_stats=(1, 0, 0))
    assert sent_to_host(loci, owner, (SIZE_TAG,), fd.CEILING, fcd.CEILING) == {2, 3, 4, 5, 6}
    assert sent_to_host(loci, owner, (SIZE_TAG,), fd.SHALLOW, fd.SHALLOW) == {2, 4, 5}


def test_statistics_refuse_a_null_out_on_a_live_context():
    """TRGT_ERR_INVALID (-1) from every statistics call, trgt_hip_snv_cluster_stats included; the context stays usable"""
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    try:
        for _, _, stats, _, _, _ in _lib.ROUTES:
            assert getattr(_lib.lib(), stats)(ctx.handle, None) == -1, stats
        assert ctx.snv_cluster_stats() == ZERO4 and ctx.flank_cluster_stats() == ZERO3
    finally:
        ctx.close()


def test_all_settings_on(locus, case, limits):
    _run(locus, case, limits, ROUTES, True)


@pytest.mark.parametrize("depth", [True, False], ids=["depth settings", "no depth settings"])
@pytest.mark.parametrize("route", ROUTES)
def test_one_setting_alone(locus, case, limits, route, depth):
    want = _run(locus, case, limits, (route,), depth)
    mine = {SIZE_TAG: "flank_stats", SIZE_SNV: "snv_split_stats", CLUSTER_TAG: "flank_cluster_stats", CLUSTER_SNV: "snv_cluster_stats",
            CLUSTER_DEEP_TAG: "flank_cluster_deep_stats"}[route]
    assert all(not any(v) for k, v in want.items() if k not in (mine, "size_deep_stats")), want
