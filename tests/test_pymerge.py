"""tests/pymerge.py, the restatement of merge_exact the merge path is held to: against the reference's own two known-answer tests
(tests/golden/merge_kats.json) and against values written out by hand for the overwrite rule and each status."""
import json
import os

import pytest

import pymerge

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_kats.json")))["cases"]
REF = b"CAGCAG"


def tup(g):
    return [(k, i) for k, i in g]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_reference_kats(case):
    assert case["source"].startswith("exact.rs:")
    gts = [[tup(sample) for sample in entry] for entry in case["vcf_gts"]]
    alleles = [[a.encode() for a in al] for al in case["sample_alleles"]]
    out_gts, merged = pymerge.merge_exact(gts, alleles)
    assert merged[0] == case["expect"]["first"].encode()
    assert len(merged) == case["expect"]["n_alleles"]
    assert len(case["expect"]["out_gts"]) == len(gts)
    for i, j, want in case["expect"]["out_gts"]:
        assert out_gts[i][j] == tup(want)


def test_kats_are_the_two_of_the_reference():
    assert [c["name"] for c in KATS] == ["test_merge_exact", "test_merge_exact_phasing"]
    assert [len(c["sample_alleles"]) for c in KATS] == [5, 2]


def test_order_is_length_then_bytes():
    out_gts, merged = pymerge.merge_exact([[[("U", 1), ("U", 2), ("P", 3), ("U", 4)]]], [[REF, b"BAAA", b"AAAB", b"T", b"AC\x80"]])
    assert merged == [REF, b"T", b"AC\x80", b"AAAB", b"BAAA"]
    assert out_gts == [[[("U", 4), ("U", 3), ("P", 1), ("U", 2)]]]
    _, merged = pymerge.merge_exact([[[]]], [[REF, b"AC\x80G", b"AC\x7fG", b"", b"ACG"]])
    assert merged == [REF, b"", b"ACG", b"AC\x7fG", b"AC\x80G"]


def test_overwrite_rule_by_hand():
    """an ALT with the bytes of the REF: the list keeps both, and everything with those bytes -- GT 0 included -- maps to the ALT's place"""
    out_gts, merged = pymerge.merge_exact([[[("U", 0), ("U", 2)]], [[("P", 0), ("P", 1)]]], [[REF, b"CAG", REF], [REF, b"CAGCAGCAG"]])
    assert merged == [REF, b"CAG", REF, b"CAGCAGCAG"]
    assert out_gts == [[[("U", 2), ("U", 2)]], [[("P", 2), ("P", 3)]]]
    assert pymerge.site_arrays([[REF, b"CAG", REF], [REF, b"CAGCAGCAG"]], [[2, 6], [3, 5]]) == (0, [0, 1, 2, 4], [2, 1, 2, 2, 3], [[6, 6], [7, 9]])


def test_statuses_by_hand():
    with pytest.raises(pymerge.MergeError, match="^Reference alleles do not match: 'CAGCAG' and 'CAGCAT'$") as e:
        pymerge.merge_exact([[[("U", 5)]], [[]], [[]]], [[REF, b"C"], [], [b"CAGCAT"]])   # (and a bad GT: the REFs come first)
    assert e.value.status == 1
    with pytest.raises(pymerge.MergeError, match="^No reference allele found$") as e:
        pymerge.merge_exact([[[("U", None)]], [[]]], [[], []])
    assert e.value.status == 2
    with pytest.raises(pymerge.MergeError, match="^No reference allele found$"):
        pymerge.merge_exact([], [])
    with pytest.raises(pymerge.MergeError, match="^Index out of bounds or allele not found in index: None$") as e:
        pymerge.merge_exact([[[("U", 1), ("P", 2)]]], [[REF, b"C"]])
    assert e.value.status == 3
    with pytest.raises(pymerge.MergeError, match="^Index out of range: -1$"):
        pymerge.merge_exact([[[("U", -1)]]], [[REF, b"C"]])
    assert pymerge.site_arrays([[REF, b"C"], [], [b"CAGCAT"]], [[12], [], []], first_allele=10) == (1, [10, 12], None, None)
    assert pymerge.site_arrays([[], []], [[0], []]) == (2, [], None, None)
    assert pymerge.site_arrays([[REF, b"C"]], [[4, 6]]) == (3, [], None, None)


def test_missing_and_phase_pass_through():
    out_gts, _ = pymerge.merge_exact([[[("U", None), ("P", None)], [("P", 1)]]], [[REF, b"C"]])
    assert out_gts == [[[("U", None), ("P", None)], [("P", 1)]]]
    assert pymerge.site_arrays([[REF, b"C"]], [[0, 1, -2147483647, 5]]) == (0, [0, 1], [0, 1], [[0, 1, -2147483647, 5]])
