"""tests/pymeth.py -- the Python restatement of get_tr_meth / assign_read / get_meth (tr.rs:198-266, 363-398) the GPU tests of
trgt_locus_meth_batch compare against -- held to hand-computed values, and tests/meth_cases.py held to being able to tell a kernel that sums
in another order from one that sums in the reference's (CPU only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meth_cases  # noqa: E402
import pymeth  # noqa: E402


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_anchor_by_hand():
    # ACGTCGCG: CpGs at 1, 4, 6 (calls 255, 0, 51); inside (2, 7): 4 and 6 -> (0/255 + 51/255) / 2 = 0.2 / 2
    assert pymeth.get_tr_meth(b"ACGTCGCG", [255, 0, 51], (2, 7)) == 0.1
    assert pymeth.get_tr_meth(b"ACGTCGCG", [255, 0, 51], (1, 2)) == 1.0   # the C at span_start counts, index 0
    assert pymeth.get_tr_meth(b"ACGTCGCG", [255, 0, 51], (2, 4)) is None  # C at span_start - 1 does not; no CpG inside
    assert pymeth.get_tr_meth(b"ACGTCGCG", [255, 0, 51], (6, 7)) == 0.2   # the last two bases of the read
    assert pymeth.get_tr_meth(b"ACGTCGCG", None, (2, 7)) is None and pymeth.get_tr_meth(b"ACGTCGCG", b"", (2, 7)) is None
    with pytest.raises(pymeth.Malformed):
        pymeth.get_tr_meth(b"ACGTCGCG", [255, 0], (2, 7))
    assert pymeth.get_tr_meth(b"ACGTCGCG", [255, 0], (2, 6)) == 0.0       # the missing call lies beyond the span: not looked at


def test_sum_order_shows_in_the_bits():
    a, b, c = 1 / 255.0, 1 / 255.0, 32 / 255.0
    assert (a + b) + c != a + (b + c)
    f, r = pymeth.get_tr_meth(b"CGCGCG", [1, 1, 32], (0, 6)), pymeth.get_tr_meth(b"CGCGCG", [1, 1, 32], (0, 6), "reversed")
    assert f == ((a + b) + c) / 3 and r == ((c + b) + a) / 3 and f != r


def test_assign_read_outcomes():
    gt = [(10, (8, 12)), (20, (18, 22))]
    assert pymeth.assign_read(gt[:1], 500) == pymeth.FIRST
    assert pymeth.assign_read(gt, 11) == pymeth.FIRST and pymeth.assign_read(gt, 19) == pymeth.SECOND
    assert pymeth.assign_read(gt, 13) == pymeth.NONE   # nearer to the first, outside its interval
    assert pymeth.assign_read(gt, 15) == pymeth.NONE   # equal distances, unequal sizes
    assert pymeth.assign_read([(12, (10, 14)), (12, (12, 12))], 13) == pymeth.BOTH
    assert pymeth.assign_read([(12, (10, 12)), (12, (12, 14))], 13) == pymeth.NONE   # Both looks at the first interval only


def test_get_meth_by_hand():
    reads = [(b"ACGT", [51]), (b"ACGTT", [102]), (b"TTTT", [1]), (b"ACG", None)]
    spans = [(0, 4), (0, 5), (0, 4), (0, 3)]
    assert pymeth.get_meth([(4, (0, 9))], reads, spans) == ([(0.2 + 0.4) / 2], [2])
    assert pymeth.get_meth([(4, (4, 4)), (5, (5, 5))], reads, spans) == ([0.2, 0.4], [1, 1])
    # output order: the swap of "reference allele first" moves level and count with the allele
    am, n, rm = pymeth.locus_meth(2, [5, 4], [5, 5, 4, 4], 1, reads, spans, [0, 1, 2, -1])
    assert am == [0.4, 0.2] and n == [1, 1] and rm[:2] == [0.2, 0.4] and all(v != v for v in rm[2:])


@pytest.mark.parametrize("name", [k for k, (_, notes) in meth_cases.CASES.items() if notes.get("order")])
def test_order_sensitive_cases_tell_orders_apart(name):
    """A case marked order-sensitive must give other bits for the reversed sum AND for a pairwise tree: a test that a reordered kernel
    passes would show nothing.  "read": the per-read sum over CpGs; "allele": the per-allele sum over reads (per-read sums left forward)."""
    loci, notes = meth_cases.CASES[name]
    which = 2 if notes["order"] == "read" else 0
    want = bits(meth_cases.expected(loci)[which])
    for mutant in ("reversed", "pairwise"):
        kw = {"order": mutant} if notes["order"] == "read" else {"allele_order": mutant}
        got = bits(meth_cases.expected(loci, **kw)[which])
        assert (got != want).any(), (name, mutant)
        if notes["order"] == "allele":  # the mutant touches only the allele sums
            assert (bits(meth_cases.expected(loci, **kw)[2]) == bits(meth_cases.expected(loci)[2])).all()


def test_many_reads_ranks_are_a_permutation_of_input_order():
    for name in ("many_reads", "many_reads_two_alleles"):
        ranks = [r["rank"] for r in meth_cases.CASES[name][0][0]["reads"]]
        assert len(ranks) > 64 and sorted(ranks) == list(range(len(ranks))) and ranks != sorted(ranks)


def test_designed_cases_cover_what_they_are_named_for():
    E = lambda name: meth_cases.expected(meth_cases.CASES[name][0], gt_size_null=meth_cases.CASES[name][1].get("gt_size_null", False))
    nan = lambda v: v != v
    assert all(nan(v) for v in E("has_meth_0")[0]) and all(nan(v) for v in E("no_cpg_in_span")[0]) and all(nan(v) for v in E("empty_span")[0])
    assert list(E("empty_range")[1]) == [1, 0] and nan(E("empty_range")[2][0])
    assert E("c_before_span")[2][0] == 20 / 255.0 and E("c_last_of_span")[2][0] == 20 / 255.0
    assert list(E("cg_ends_read")[2][:2]) == [77 / 255.0, 5 / 255.0] and nan(E("cg_ends_read")[2][2])
    assert list(E("boundaries")[2][:3]) == [((1 / 255.0 + 1 / 255.0) + 32 / 255.0) / 3, (200 / 255.0 + 31 / 255.0) / 2, (9 / 255.0 + 200 / 255.0) / 2]
    assert E("anchor")[0][0] == 0.1
    assert list(E("nearer_outside_interval")[1]) == [1, 0] and list(E("equal_sizes_both")[1]) == [2, 2] and list(E("equal_distance_unequal_sizes")[1]) == [1, 1]
    assert list(E("no_alleles")[1]) == [0, 0] and list(E("no_kept_reads")[1]) == [0, 0, 0, 0, 1, 1]
    # gt_size decides where allele_len would decide otherwise, and the NULL form falls back to allele_len
    g, gn = meth_cases.CASES["gt_size_differs"][0], meth_cases.CASES["gt_size_null"][0]
    assert list(meth_cases.expected(g)[1]) != list(meth_cases.expected(g, gt_size_null=True)[1])
    assert list(meth_cases.expected(gn)[1]) != list(meth_cases.expected(gn, gt_size_null=True)[1])
    with pytest.raises(pymeth.Malformed):
        meth_cases.expected(meth_cases.CASES["malformed_in_span"][0])
    meth_cases.expected(meth_cases.CASES["short_calls_beyond_span"][0])   # no error
    # more than 64 CpGs in one span
    mb = meth_cases.CASES["many_cpg"][0][0]["reads"][0]
    assert sum(1 for p in range(mb["span"][0], mb["span"][1]) if mb["bases"][p:p + 2] == b"CG") > 64


def test_wrong_order_mutant_is_caught_by_the_cases():
    """What the GPU test does with the kernel's output, done here with a mutant in the kernel's place: comparing bits over all cases
    catches a per-read reordering and a per-allele reordering alike."""
    def run(**kw):
        out = []
        for name, (loci, notes) in meth_cases.CASES.items():
            if "error" not in notes:
                e = meth_cases.expected(loci, gt_size_null=notes.get("gt_size_null", False), **kw)
                out.append(np.concatenate([bits(e[0]), bits(e[2])]))
        return np.concatenate(out)
    want = run()
    assert (run() == want).all()
    for kw in ({"order": "reversed"}, {"order": "pairwise"}, {"order": "forward", "allele_order": "reversed"}, {"order": "forward", "allele_order": "pairwise"}):
        assert (run(**kw) != want).any(), kw


def test_pack_and_split_batch_carry_the_calls():
    """locus.pack takes a per-locus "meth" list (None or bytes per read); driver.split_batch re-bases the three arrays per chunk"""
    from trgt_amd import driver, locus
    mk = lambda reads, meth: dict(left_flank=b"A" * 4, right_flank=b"C" * 4, tr=b"CAG", motifs=[b"CAG"], reads=reads, **({"meth": meth} if meth is not None else {}))
    loci = [mk([b"ACGT", b"CGCG"], [b"\x07", None]), mk([b"TT"], None), mk([b"CGA", b"ACG", b"A"], [b"", b"\x09\x0a", b"\x01"])]
    b = locus.pack(loci)
    assert list(b["has_meth"]) == [1, 0, 0, 1, 1, 1] and list(b["meth_off"]) == [0, 1, 1, 1, 1, 3, 4] and bytes(b["meth"]) == b"\x07\x09\x0a\x01"
    assert "meth" not in locus.pack([mk([b"ACGT"], None)])
    chunks = driver.split_batch(b, 2)
    assert [list(c["meth_off"]) for c in chunks] == [[0, 1, 1, 1], [0, 0, 2, 3]] and [list(c["has_meth"]) for c in chunks] == [[1, 0, 0], [1, 1, 1]]
    assert [bytes(c["meth"][:int(c["meth_off"][-1])]) for c in chunks] == [b"\x07", b"\x09\x0a\x01"]
    assert "meth" not in driver.split_batch(locus.pack([mk([b"ACGT"], None)]), 1)[0]


def test_bam4_packing_of_the_cases():
    assert meth_cases.pack_bam4(b"ACGTN") == bytes([0x12, 0x48, 0xF0])
    b = meth_cases.build(meth_cases.CASES["cg_ends_read"][0], encoding=1, lead=3)
    assert list(b["read_off"]) == [3, 6, 7] and list(b["read_len"]) == [6, 2, 3]
