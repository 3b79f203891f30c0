"""filter_impure_trs (src/trgt/workflows/tr.rs:400-452) as arithmetic: the f64::total_cmp key, the stable order and the walk with its
budget max(1, round(0.1 n)), restated in a few lines of Python (tests/purity_cases.py) and held against the oracle on the loci the
device test uses.  purity_filter_kernel restates the same three things, so a disagreement on the GPU can be put down to the kernel
or to the reading of tr.rs."""
import numpy as np
import pytest

import purity_cases as pc


def _kept_by_restatement(oracle, L):
    # the selection in front of the filter is get_spanning_reads: the oracle's own kept list with the filter off
    kw = dict(ploidy=L.get("ploidy", 2), genotyper=1 if L.get("genotyper") == "cluster" else 0)
    sel = oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], **kw)
    pur = []
    for r in (int(v) for v in sel["kept_read"]):
        rq = L["read_qual"][r]
        if rq is not None and rq >= 0.9:
            pur.append(1.0)
        else:
            s, e = int(sel["span_start"][r]), int(sel["span_end"][r])
            pur.append(float(oracle.hmm_annotate(L["motifs"], L["reads"][r][s:e])["purity"]))
    keep = pc.filter_order(pur)
    return [int(sel["kept_read"][i]) for i in keep], pur, kw


@pytest.mark.parametrize("maker", [pc.budget_loci, pc.ordering_loci, pc.nan_loci, pc.no_majority_loci])
def test_restated_filter_matches_oracle(oracle, maker):
    for l, L in enumerate(maker()):
        want, pur, kw = _kept_by_restatement(oracle, L)
        rq = [np.nan if q is None else q for q in L["read_qual"]]
        ref = oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], min_read_qual=0.5, read_qual=rq, **kw)
        assert [int(v) for v in ref["kept_read"]] == want, (maker.__name__, l, pur)


def test_budget_rounds_half_away_from_zero():
    assert [pc.max_filter(n) for n in (1, 4, 5, 14, 15, 16, 25, 26, 35, 250)] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 25]


def test_total_cmp_key_orders_like_total_cmp():
    neg_nan = float(np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0])
    xs = [neg_nan, -np.inf, -1.0, -0.0, 0.0, 0.5, 0.8999999999999999, 0.9, 1.0, np.inf, float("nan")]
    keys = [pc.total_cmp_key(x) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_cases_do_what_they_are_there_for(oracle):
    """the loci must exercise the filter: reads dropped up to the budget and not beyond, NaN purities present, ties present"""
    dropped = []
    for L in pc.budget_loci():
        want, pur, _ = _kept_by_restatement(oracle, L)
        n_bad = sum(not (p >= 0.9) for p in pur)
        assert n_bad > pc.max_filter(len(pur)) or len(pur) == 4
        dropped.append(len(pur) - len(want))
    assert dropped == [1, 1, 2, 3, 1]
    want, pur, _ = _kept_by_restatement(oracle, pc.ordering_loci()[0])
    assert len(set(pur)) < len(pur) - 3 and len(want) == len(pur) - 1
    want, pur, _ = _kept_by_restatement(oracle, pc.ordering_loci()[2])
    assert pur == [1.0] * 7 and len(want) == 7
    nan = pc.nan_loci()
    for L, n_nan, n_drop in zip(nan, (1, 1, 3), (1, 1, 1)):
        want, pur, _ = _kept_by_restatement(oracle, L)
        assert sum(np.isnan(p) for p in pur) == n_nan and len(pur) - len(want) == n_drop, pur
    # with the budget spent on the impure read in front of it, the NaN read stays
    want, pur, _ = _kept_by_restatement(oracle, nan[1])
    assert any(np.isnan(pur[i]) for i in pc.filter_order(pur))
