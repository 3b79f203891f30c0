"""The SNV branch of genotype_flank inside the device genotyper (trgt_hip_set_snv_split_device; locus_gt.hpp, SNV forms): every case of
snv_split_cases.py against the oracle, on a context with the setting alone, with set_flank_device(True) as well, as it is created, and
under TRGT_HOST_GENOTYPER.  trgt_hip_snv_split_stats must be what the plain-Python restatement of the branch predicts (the conditions of
the cases: test_snv_split_cases.py)."""
import numpy as np
import pytest

import snv_split_cases as sc
from test_flank_device_gpu import _compare, _ref, _runs

pytestmark = pytest.mark.gpu
ZERO = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def ctxs():
    from trgt_amd import _lib
    alone, both, off, host = _lib.Context(0), _lib.Context(0), _lib.Context(0), _lib.context_with_env(TRGT_HOST_GENOTYPER=1)
    alone.set_snv_split_device(True)
    both.set_snv_split_device(True)
    both.set_flank_device(True)
    yield [("alone", alone), ("both", both), ("off", off), ("host genotyper", host)]
    for c in (alone, both, off, host):
        c.close()


def _check(oracle, locus, ctxs, loci, params=None, handed=(), want=None, flank_want=None, on_ctx=None):
    """want: what the case itself expects of trgt_hip_snv_split_stats; flank_want: of trgt_hip_flank_stats per context name"""
    params = params or locus.Params()
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = [_ref(oracle, L, params, meta=False) for L in loci]
    stats = sc.expected_stats(loci, plain, handed)
    if want is not None:
        assert stats == want
    flipped = []
    for name, ctx in ([("alone", on_ctx)] if on_ctx is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            if name != "host genotyper":
                print(name, how, "snv_split_stats", ctx.snv_split_stats(), "expected", stats if name in ("alone", "both") else ZERO, "flank_stats", ctx.flank_stats())
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            if name != "host genotyper":
                assert ctx.snv_split_stats() == (stats if name in ("alone", "both") else ZERO), (name, how)
                if flank_want is not None:
                    assert ctx.flank_stats() == flank_want.get(name, ZERO), (name, how)
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, stats


def test_reference_vectors(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, sc.case_kats(), want=(1, 0, 0, 0), flank_want={})
    assert [int(v) for v in refs[0]["classification"]] == [0, 0, 0, 1, 1, 1]


def test_plain_split(oracle, locus, ctxs):
    _, _, stats = _check(oracle, locus, ctxs, sc.case_plain(), flank_want={})
    assert stats[0] == 1


@pytest.mark.parametrize("n", [3, 10, 30])
def test_skip_rounding(oracle, locus, ctxs, n):
    _check(oracle, locus, ctxs, sc.case_skip(n)[0], want=(2, 0, 0, 0))


def test_call_threshold_and_fewest_fully_observed_reads(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_call_threshold() + sc.case_least_full(), want=(2, 0, 0, 0))


def test_ties_in_the_assignment(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, sc.case_ties(), want=(1, 0, 0, 0))
    assert sc.Y60.decode() in refs[0]["alleles"]


def test_last_maximum_and_margin(oracle, locus, ctxs):
    loci = sc.case_margin()
    _check(oracle, locus, ctxs, loci[:2], want=(0, 0, 0, 2), flank_want={})
    _check(oracle, locus, ctxs, loci, want=(1, 0, 0, 2))


def test_repair_swap_and_reference_first(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, sc.case_repair(), want=(4, 2, 0, 0))
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs[:2])


@pytest.mark.parametrize("env", [dict(TRGT_REPAIR_MAX_SEG=60), dict(TRGT_HOST_REPAIR=1)])
def test_handing_back(oracle, locus, ctxs, env):
    from trgt_amd import _lib
    ctx = _lib.context_with_env(**env)
    try:
        ctx.set_snv_split_device(True)
        _check(oracle, locus, ctxs, sc.case_hand_back(), handed=(0,), want=(1, 0, 1, 0), flank_want={}, on_ctx=ctx)
    finally:
        ctx.close()


def test_large_instantiation(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_forms(), want=(3, 0, 0, 0))


@pytest.mark.parametrize("n,big", [(20, False), (40, True)])
def test_segments_that_do_not_fit_the_lds(oracle, locus, ctxs, n, big):
    _check(oracle, locus, ctxs, sc.case_segments_beyond_lds(n, big), want=(2 if big else 1, 0, 0, 0))


def test_purity_filter_on(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, sc.case_purity(), params=locus.Params(min_read_qual=0.5), want=(3, 0, 0, 0))


@pytest.mark.parametrize("case", ["snv", "hap", "offset small", "offset big"])
def test_limits(oracle, locus, ctxs, case):
    loci = {"snv": sc.case_snv_cap, "hap": sc.case_hap_cap, "offset small": lambda: sc.case_offset_cap(False), "offset big": lambda: sc.case_offset_cap(True)}[case]()
    _check(oracle, locus, ctxs, loci, want=(1, 0, 1, 0), flank_want={})  # at the cap: settled; one beyond: handed back


def test_tags_and_snvs_together(oracle, locus, ctxs):
    # the tags of [0] split: the tag route where both settings are on, the host where this one is alone (no count anywhere);
    # [1] is the SNV route's on both
    _check(oracle, locus, ctxs, sc.case_tags_and_snvs(), want=(1, 0, 0, 0), flank_want={"both": (1, 0, 0, 0)})


def test_mixed_batch(oracle, locus, ctxs):
    # (the cluster locus is the host's: its own flank step finds the split and sends it, which flank_stats()[2] keeps counting where
    #  set_flank_device is on)
    _, _, stats = _check(oracle, locus, ctxs, sc.case_mixed(), flank_want={"both": (0, 0, 1, 0)})
    assert stats[0] == 3 and stats[2:] == (0, 0)


def test_random_loci(oracle, locus, ctxs):
    _, _, stats = _check(oracle, locus, ctxs, sc.case_random())
    assert stats[3] <= 2


def test_other_entry_points(oracle, locus, ctxs):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = ctxs[0][1]
    loci = sc.case_kats() + sc.case_repair() + sc.case_margin()
    b, refs, stats = _check(oracle, locus, ctxs, loci, on_ctx=on)
    assert stats == (6, 2, 0, 2)
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, ctx=on))
    assert recs(b, locus.submit_batch(b, ctx=on).wait()) == want and on.snv_split_stats() == stats
    got, total = [], [0, 0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, ctx=on))
        total = [x + y for x, y in zip(total, on.snv_split_stats())]
    assert got == want and tuple(total) == stats
    pool = _lib.Pool([0, 0], snv_split_device=True)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
        assert tuple(sum(c.snv_split_stats()[k] for c in pool.contexts) for k in range(4))[0] > 0
    finally:
        pool.close()
    # the setting on a batch without mismatch arrays: nothing to do, nothing counted
    plain = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    ref_plain = [_ref(oracle, L, locus.Params(), meta=False) for L in loci]
    _compare(locus, plain, locus.run_batch(plain, ctx=on, reads_dev=torch.from_numpy(plain["read_blob"]).cuda()), ref_plain, "no mismatch arrays")
    assert on.snv_split_stats() == ZERO
