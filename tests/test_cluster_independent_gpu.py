"""The three product copies of the Ward linkage -- the host path (locus_cluster.hpp: ward_nnchain), the one-wave kernel in both
instantiations (locus_cluster_dev.hpp: cluster_ward_kernel <64, LDS matrix> and <256, HBM matrix>) and the deep chain
(locus_cluster_deep.hpp) -- held to tests/pyward.py through trgt_locus_batch, on the designed loci of tests/cluster_cases.py: tie-heavy
matrices at the sizes where the copies differ.  tests/test_cluster_independent.py (no GPU) holds the oracle to the same restatement and
shows that the `sensitive` lists detect the altered readings of the rules; every route here runs the lists of its sizes, and two of the
readings are switched on in the one-wave kernels (developer build) and must be seen.

Every result is compared with the restatement's classification and, field by field as tests/test_cluster_deep_gpu.py does, with the
oracle, whose result of a locus is computed once per process.  Every route runs with host reads and with reads resident in HBM."""
import pytest

import cluster_cases as cc
from test_cluster_deep_gpu import _compare, _runs

pytestmark = pytest.mark.gpu

DEVICE_RULES = {"ties_last": "TRGT_SENS_WARD_TIES", "lw_order": "TRGT_SENS_LW_ORDER"}  # (ClArgs::flags: the one-wave kernels only)


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def _lib():
    from trgt_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def plain_ctx(_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def deep_ctx(_lib):
    ctx = _lib.Context(0)
    ctx.set_cluster_max_reads(_lib.cluster_max_reads_limit())
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host_ctx(_lib):
    ctx = _lib.context_with_env(TRGT_HOST_CLUSTER=1)
    yield ctx
    ctx.close()


def _designed(lo, hi):
    """the designed lists and the `sensitive` lists of every altered rule (the loci on which tests/test_cluster_independent.py shows a
    kernel that took that rule to give another classification): every route is held to the restatement on both"""
    cases = [c for cases in cc.all_lists().values() for c in cases]
    for rule in sorted(cc.RULES):
        for size_class in cc.SIZE_CLASSES:
            assert len(cc.sensitive(rule, size_class)) >= cc.FLOORS[size_class], (rule, size_class)
            cases += [c for c in cc.sensitive(rule, size_class) if c not in cases]  # (one seed may serve several rules)
    return [c for c in cases if lo <= c.n <= hi]


def _has_sensitive(cases, *size_classes):
    return all(set(cc.sensitive(rule, size_class)) <= set(cases) for rule in cc.RULES for size_class in size_classes)


_RESTATED = {}


def _restated(oracle, case):
    if case.name not in _RESTATED:
        _RESTATED[case.name] = cc.answer(case, (), None if case.equal_lengths else cc.oracle_ref(oracle, case))
    return _RESTATED[case.name]


def _check(oracle, locus, cases, ctx, on_device):
    """on_device: how many of the loci a device chain must report (stats[22]), none of them sent back for want of room (stats[23])"""
    b = locus.pack([cc.locus(c) for c in cases])
    refs = [cc.oracle_ref(oracle, c) for c in cases]
    params = locus.Params(max_depth=cc.MAX_DEPTH)
    for mode, out in _runs(locus, b, params, ctx):
        assert int(out.stats[22]) == on_device and int(out.stats[23]) == 0, (mode, out.stats[22:24])
        for l, case in enumerate(cases):
            assert locus.locus_result(b, out, l).classification == _restated(oracle, case).classification, (mode, case)
        _compare(locus, b, out, refs)


def test_one_wave_lds_matrix(oracle, locus, plain_ctx):
    cases = _designed(2, 64)
    assert {3, 4, 5, 63, 64} <= {c.n for c in cases} and _has_sensitive(cases, "lds")
    _check(oracle, locus, cases, plain_ctx, len(cases))


def test_one_wave_hbm_matrix(oracle, locus, plain_ctx):
    cases = _designed(65, 256)
    assert {65, 128, 129, 255, 256} <= {c.n for c in cases} and _has_sensitive(cases, "hbm")
    _check(oracle, locus, cases, plain_ctx, len(cases))


def test_deep_chain(oracle, locus, deep_ctx):
    # 257 is the first locus the deep chain takes; 256 stays with the one-wave kernel on the same context
    cases = _designed(257, 10 ** 6)
    assert {257, 300, 330, 350} <= {c.n for c in cases} and _has_sensitive(cases, "deep")
    _check(oracle, locus, cases, deep_ctx, len(cases))
    _check(oracle, locus, [c for c in _designed(255, 257) if c.name.startswith("random_hamming")], deep_ctx, 3)


def test_host_path_up_to_256(oracle, locus, host_ctx):
    cases = _designed(2, 256)
    assert _has_sensitive(cases, "lds", "hbm")
    _check(oracle, locus, cases, host_ctx, 0)


def test_host_path_beyond_256(oracle, locus, host_ctx, plain_ctx):
    cases = _designed(257, 10 ** 6)
    assert _has_sensitive(cases, "deep")
    _check(oracle, locus, cases, host_ctx, 0)
    _check(oracle, locus, [c for c in _designed(257, 257)], plain_ctx, 0)  # the setting at its default: a deep locus is the host path's


@pytest.mark.parametrize("rule", sorted(DEVICE_RULES))
def test_altered_rule_is_seen_on_the_device(oracle, locus, _lib, plain_ctx, rule):
    """The one-wave kernels with one rule altered give the restatement's classification under the same rule, which is not the default
    context's on any of these loci (tests/test_cluster_independent.py asserts that of the restatement and the oracle)."""
    altered_ctx = _lib.context_with_env(**{DEVICE_RULES[rule]: 1})
    try:
        cases = list(cc.sensitive(rule, "lds") + cc.sensitive(rule, "hbm"))
        assert len(cases) >= cc.FLOORS["lds"] + cc.FLOORS["hbm"]
        b = locus.pack([cc.locus(c) for c in cases])
        refs = [cc.oracle_ref(oracle, c) for c in cases]
        params = locus.Params(max_depth=cc.MAX_DEPTH)
        for (mode, plain), (_, altered) in zip(_runs(locus, b, params, plain_ctx), _runs(locus, b, params, altered_ctx)):
            assert int(plain.stats[22]) == int(altered.stats[22]) == len(cases), mode
            assert int(plain.stats[23]) == int(altered.stats[23]) == 0, mode
            _compare(locus, b, plain, refs)
            for l, case in enumerate(cases):
                want, got = cc.altered_answer(case, rule), locus.locus_result(b, altered, l)
                assert got.classification == want.classification, (mode, case)
                assert tuple(a.seq for a in got.genotype) == want.alleles, (mode, case)
                assert locus.locus_result(b, plain, l).classification == _restated(oracle, case).classification != got.classification, (mode, case)
    finally:
        altered_ctx.close()


def test_answers_follow_the_loci(oracle, locus, deep_ctx):
    """one batch in which loci of all size classes and size-genotyper loci alternate, and the same loci in reversed order"""
    cases = [c for d in ("hypercube", "random_hamming") for c in cc.design_list(d) if c.n in (5, 64, 65, 256, 257, 330)]
    cases += [c for name in ("negative_cutoff", "dropped_reads", "max_ops_edge", "outlier_redo") for c in cc.special_list(name)]
    loci, refs = [], []
    for k, case in enumerate(cases):
        L = cc.locus(case)
        loci.append(L)
        refs.append(cc.oracle_ref(oracle, case))
        if k % 2 == 0:  # the same reads under Genotyper::Size
            loci.append(dict(L, genotyper="size"))
            refs.append(oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], genotyper=0, max_depth=cc.MAX_DEPTH))
    params = locus.Params(max_depth=cc.MAX_DEPTH)
    for order in (list(range(len(loci))), list(range(len(loci) - 1, -1, -1))):
        b = locus.pack([loci[i] for i in order])
        for mode, out in _runs(locus, b, params, deep_ctx):
            assert int(out.stats[22]) == len(cases) and int(out.stats[23]) == 0, (mode, out.stats[22:24])
            _compare(locus, b, out, [refs[i] for i in order])
