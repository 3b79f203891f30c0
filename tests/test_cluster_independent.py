"""The CPU oracle's cluster genotyper (oracle/locus.cpp: ward_linkage, cluster, genotype) held to tests/pyward.py, a restatement written
from the reference and the published definitions alone, on the tie-heavy matrices of tests/cluster_cases.py -- sqrt(small integer), where
the result depends on which of several equal neighbours is taken, on a tie keeping the previous chain element, on the order of the f64
operations of the Lance-Williams update, on which row survives a merge and on the stability of the sort of the merges.  No GPU.

Every comparison is of integers or of f64 bit patterns.  The one tolerance, 1e-9 relative, is that of
test_oracle_cluster.py::test_ward_dendrogram_matches_scipy and applies to the exact anchor alone: tie-free matrices whose dendrogram is
unique, where the restatement itself is held to the primitive algorithm in exact arithmetic.

tests/test_cluster_independent_gpu.py runs the same loci through the host path and both device chains."""
import math

import numpy as np
import pytest

import cluster_cases as cc
import pyward
import pywfa


def _bits(values):
    return np.asarray(values, np.float64).tobytes()


def test_edit_distances_of_the_case_builder():
    """the builder's vectorised table against the plain DP of pywfa on a sample of every kind of pair, equal and unequal lengths; the
    designs keep substitution sites apart so that a pair's edit distance is its Hamming distance, which is counted here, not assumed"""
    rng = np.random.default_rng(5)
    pairs = []
    for case in (cc.design_list("random_hamming")[4], cc.design_list("chain")[1], cc.design_list("three_centres")[0]) + cc.special_list("max_ops_edge") + cc.special_list("negative_cutoff"):
        s = case.sorted_segs
        for _ in range(20):
            i, j = sorted(int(v) for v in rng.choice(case.n, size=2, replace=False))
            if len(s[i]) * len(s[j]) <= pyward.MAX_OPS:
                assert case.scores[pyward.pair_index(case.n, i, j)] == pywfa.optimum(s[i], s[j], "edit"), (case, i, j)
                pairs.append((s[i], s[j]))
    assert len(pairs) >= 60  # (the three lists of equal lengths alone give 60)
    hamming = sum(1 for a, b in pairs if len(a) == len(b) and pywfa.optimum(a, b, "edit") == sum(x != y for x, y in zip(a, b)))
    assert hamming >= 40


@pytest.mark.parametrize("name", sorted(cc.DESIGNS) + list(cc.SPECIAL) + ["sensitive"])
def test_oracle_linkage_and_groups_equal_the_restatement(oracle, name):
    """steps, sizes, dissimilarities and the matrix as the call leaves it, bit for bit; cluster()'s groups"""
    if name == "sensitive":
        cases = [c for rule in cc.RULES for size_class in cc.SIZE_CLASSES for c in cc.sensitive(rule, size_class)]
    else:
        cases = cc.all_lists()[name]
    assert cases
    for case in cases:
        n, d = case.n, case.dists()
        if n >= 3:
            st, di, mutated = oracle.ward_linkage(d, n)
            steps, mat = pyward.linkage(list(d), n)
            assert len(steps) == n - 1 == len(st), case
            assert [(s[0], s[1], s[3]) for s in steps] == [tuple(int(v) for v in row) for row in st], case
            assert _bits([s[2] for s in steps]) == di.tobytes(), case
            assert _bits(mat) == mutated.tobytes(), case
        k, g, mutated = oracle.cluster_groups(d, n)
        mine = list(d)
        groups = pyward.cluster(mine, n)
        of = [None] * n
        for gi, members in enumerate(groups):
            for r in members:
                of[r] = gi
        assert k == len(groups) and g.tolist() == of, case
        if n >= 3:
            assert _bits(mine) == mutated.tobytes(), case


def _leaves(steps, n):
    sets = [frozenset([i]) for i in range(n)]
    for c1, c2, _, size in steps:
        sets.append(sets[c1] | sets[c2])
        assert len(sets[-1]) == size
    return sets


def test_exact_anchor(oracle):
    """Tie-free integer matrices (squared distances of random integer points): exact() meets no tie and a relative gap of more than 1e-6
    between the best and the second-best pair at every step, so the dendrogram is unique and rounding decides nothing.  The restatement,
    under every reading of the rules, and the oracle produce its merges as sets of leaves, heights within 1e-9 relative."""
    used = 0
    for seed in range(130):
        rng = np.random.default_rng([seed, 11])
        n = int(rng.integers(4, 11))
        pts = rng.integers(0, 200, size=(n, 3))
        k = [int(((pts[i] - pts[j]) ** 2).sum()) for i in range(n) for j in range(i + 1, n)]
        merges, tie, gap = pyward.exact(k, n)
        if tie or gap is None or not gap > 1e-6:
            continue
        used += 1
        d = [math.sqrt(float(v)) for v in k]
        st, di, _ = oracle.ward_linkage(d, n)
        candidates = [pyward.linkage(list(d), n, **rules)[0] for rules in [{}] + list(cc.RULES.values())]
        candidates.append([(int(r[0]), int(r[1]), float(h), int(r[2])) for r, h in zip(st, di)])
        for steps in candidates:
            sets = _leaves(steps, n)
            assert len(steps) == len(merges) == n - 1
            for (c1, c2, diss, _), (a, b, height) in zip(steps, merges):
                assert {sets[c1], sets[c2]} == {a, b}, (seed, steps, merges)
                want = math.sqrt(float(height))
                assert abs(diss - want) <= 1e-9 * want, (seed, diss, want)
    assert used >= 100, used


def test_altered_rules_change_the_answer(oracle):
    """On the `sensitive` lists the restatement under the altered rule gives another classification than the oracle: a kernel that took
    that rule would fail tests/test_cluster_independent_gpu.py on these loci.  The floors: 5 loci per rule in either one-wave size class,
    3 per rule at 257-330 reads."""
    for rule in cc.RULES:
        for size_class, (lo, hi) in cc.SIZE_CLASSES.items():
            cases = cc.sensitive(rule, size_class)
            changed = 0
            for case in cases:
                assert lo <= case.n <= hi, case
                ref = cc.oracle_ref(oracle, case)
                assert ref["classification"].tolist() == cc.default_answer(case).classification, case
                changed += cc.altered_answer(case, rule).classification != ref["classification"].tolist()
            assert changed == len(cases) >= cc.FLOORS[size_class], (rule, size_class, changed)


def test_every_branch_is_reached(oracle):
    total = pyward.Counters()
    for cases in cc.all_lists().values():
        for case in cases:
            c = cc.answer(case, (), None if case.equal_lengths else cc.oracle_ref(oracle, case)).counters
            for f in total.FIELDS:
                setattr(total, f, getattr(total, f) + getattr(c, f))
    for f in ("even_odd", "negative_cutoff", "outlier_redo", "dropped_tie", "dropped_no_tie", "swap", "chain_reentry", "tie_keeps_previous", "zero_merges"):
        assert getattr(total, f) >= 1, total.as_dict()
    # what the lists were designed to reach, case by case
    answers = {c.name: cc.answer(c, (), None if c.equal_lengths else cc.oracle_ref(oracle, c)) for name in cc.SPECIAL for c in cc.special_list(name)}
    assert answers["negative_cutoff-5"].counters.negative_cutoff == 1 and len(answers["negative_cutoff-5"].groups) == 5
    assert [answers["outlier_redo-%d-5" % b].redo for b in (20, 21)] == [False, True]
    for n, need in ((150, 2), (250, 3), (350, 4)):
        short, exact = answers["min_cluster_rounding-%d-%d" % (n, need - 1)], answers["min_cluster_rounding-%d-%d" % (n, need)]
        assert short.counters.even_odd == 1 and not short.redo and short.classification == [1 - i % 2 for i in range(n)]
        assert exact.counters.even_odd == 0 and exact.redo and len(exact.group2) == need and exact.classification == [i % 2 for i in range(n)]
    tie, nearer = answers["dropped_reads-tie"], answers["dropped_reads-nearer"]
    assert (tie.counters.dropped_tie, tie.counters.dropped_no_tie) == (1, 0) and (nearer.counters.dropped_tie, nearer.counters.dropped_no_tie) == (0, 1)
    assert tie.classification.count(0) == 8 and nearer.classification.count(1) == 6
    assert all(answers["max_ops_edge-" + t].counters.swap == 1 for t in ("100-101", "80-125-126"))


@pytest.mark.parametrize("name", sorted(cc.DESIGNS) + list(cc.SPECIAL))
def test_oracle_loci_equal_the_restatement(oracle, name):
    """oracle.locus_analyze on the designed loci: the spans are the segments, the kept reads are the case's order, the alleles are the
    restated consensus, the classification is pyward.classify's, fed with the case's matrix and the oracle's allele lengths, and the number
    of edit-distance alignments is the number of pairs -- and of dropped reads against alleles -- with |a| * |b| <= MAX_OPS.  Where a group
    has members of unequal lengths -- the larger group of either max_ops_edge case, no other -- the restatement has no consensus and
    cluster_cases.allele_of hands the oracle's allele back: for that allele the comparison is the oracle against itself, and only the
    classification, the kept reads and n_wfa_ed are checked independently."""
    unequal = []
    for case in cc.all_lists()[name]:
        ref, L = cc.oracle_ref(oracle, case), cc.locus(case)
        assert [L["reads"][r][int(ref["span_start"][r]):int(ref["span_end"][r])] for r in range(case.n)] == case.segs, case
        assert ref["kept_read"].tolist() == case.order, case
        ans = cc.answer(case, (), ref)
        unequal += [case for g in (ans.group1, ans.group2) if len({len(case.sorted_segs[i]) for i in g}) > 1]
        assert ref["n_alleles"] == 2 and tuple(a.encode() for a in ref["alleles"]) == ans.alleles, case
        assert ref["classification"].tolist() == ans.classification, case
        assert ref["stats"]["n_wfa_ed"] == ans.n_ed, case
        if name == "max_ops_edge":
            pairs = {tuple(sorted((len(a), len(b)))): al for a in case.segs for b in case.segs for al in [len(a) * len(b) <= pyward.MAX_OPS]}
            assert all(pairs[k] == v for k, v in {(100, 100): True, (100, 101): False, (80, 125): True, (80, 126): False}.items() if k in pairs)
            assert case.order != list(range(case.n))  # (the sort by length permutes the reads)
    assert len(unequal) == (2 if name == "max_ops_edge" else 0), unequal  # one group of either case: see the docstring
    if name == "max_ops_edge":
        seen = {tuple(sorted((len(a), len(b)))) for case in cc.all_lists()[name] for a in case.segs for b in case.segs}
        assert {(100, 100), (100, 101), (80, 125), (80, 126)} <= seen
