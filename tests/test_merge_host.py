"""The merge path without a GPU: trgt_merge_exact_host and trgt_amd.merge.merge_exact(ctx=None) against tests/pymerge.py on every designed
case and 2 000 random sites, every output array and the reference's messages; the call errors; the loader's MERGE_EXPORTS against the
header."""
import json
import os
import re

import numpy as np
import pytest

import merge_cases
import pymerge
from trgt_amd import _lib, merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = merge.site_alleles_limit()
DESIGNED = merge_cases.designed(LIMIT)
ALL = [s for _, s in DESIGNED]
# the designed sites with sites that carry a status in between
MIXED = [x for i, s in enumerate(ALL) for x in ((s, ALL[20 + i % 6]) if i % 3 == 0 else (s,))]


def run_host(sites, pad=(0,), fill=0x5A):
    b = merge.pack(sites, pad=pad)
    outs = merge.alloc_outputs(b, fill=fill)
    merge.call(b, outs, None)
    return b, outs


def test_exports_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trgt_hip_merge.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(trgt_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.MERGE_EXPORTS)
    main_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trgt_hip.h")).read(), flags=re.S)
    assert '#include "trgt_hip_merge.h"' in main_h and main_h.index('extern "C"') < main_h.index('#include "trgt_hip_merge.h"')
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.MERGE_EXPORTS)
    assert not set(_lib.MERGE_EXPORTS) & set(_lib.EXPORTS)
    assert L.trgt_hip_abi_version() == 11
    assert LIMIT >= 4096


@pytest.mark.parametrize("name,site", DESIGNED, ids=[n for n, _ in DESIGNED])
def test_designed_case(name, site):
    for pad in ((0,), merge_cases.PAD):
        b, outs = run_host([site], pad=pad)
        merge_cases.check_outputs(b, outs, [site], name)


def test_designed_cases_cover_every_status_and_the_ties():
    got = [st for st, _, _, _ in merge_cases.expected(ALL)]
    assert {0, 1, 2, 3} == set(got)
    assert [st for st, _, _, _ in merge_cases.expected(ALL)[20:26]].count(0) < 6
    assert sum(merge_cases.has_hbm_tie(s) for s in ALL) >= 6


def test_all_designed_in_one_call():
    b, outs = run_host(MIXED, pad=merge_cases.PAD)
    merge_cases.check_outputs(b, outs, MIXED, "mixed")


def test_random_sites():
    b, outs = run_host(merge_cases.RANDOM, pad=merge_cases.PAD)
    merge_cases.check_outputs(b, outs, merge_cases.RANDOM, "random")


def as_tuples(site):
    alleles, gts = site
    return [[[merge.gt_decode(v) for v in g if v != merge.VECTOR_END]] for g in gts], [list(al) for al in alleles]


def test_merge_exact_signature_and_messages():
    sites = [s for _, s in DESIGNED[:30]] + merge_cases.RANDOM[:300]
    seen = set()
    for site in sites:
        gts, alleles = as_tuples(site)
        try:
            want = pymerge.merge_exact(gts, alleles)
        except pymerge.MergeError as e:
            with pytest.raises(ValueError) as got:
                merge.merge_exact(gts, alleles)
            assert str(got.value) == str(e)
            seen.add(e.status)
            continue
        assert merge.merge_exact(gts, alleles) == want
        seen.add(0)
    assert seen == {0, 1, 2, 3}
    with pytest.raises(ValueError, match="^Index out of range: -3$"):
        merge.merge_exact([[[("U", 1), ("P", -3)]]], [[b"CAG", b"C"]])


def test_reference_kats_through_the_library():
    for case in json.load(open(os.path.join(ROOT, "tests", "golden", "merge_kats.json")))["cases"]:
        gts = [[[(k, i) for k, i in sample] for sample in entry] for entry in case["vcf_gts"]]
        out_gts, merged = merge.merge_exact(gts, [[a.encode() for a in al] for al in case["sample_alleles"]])
        assert merged[0] == case["expect"]["first"].encode() and len(merged) == case["expect"]["n_alleles"]
        for i, j, want in case["expect"]["out_gts"]:
            assert out_gts[i][j] == [(k, v) for k, v in want]


def test_exact_batch_returns_sequences():
    res = merge.exact_batch([DESIGNED[8][1], ([[b"CAG", b"C"], [b"CAT"]], [[2], [2]]), ([], [])])
    assert res[0] == (0, [merge_cases.REF, b"AAAB", b"BAAA"], [[2, 6], [4, 4], [4, 7]])
    assert res[1] == (1, [b"CAG", b"CAT"], None) and res[2] == (2, [], None)
    assert merge.exact_batch([]) == []


SITE = ([[b"CAGCAG", b"CAG"], [b"CAGCAG", b"CA", b"CAGCA"]], [[2, 4], [4, 6]])


def broken(what):
    b = merge.pack([SITE, SITE])
    outs = merge.alloc_outputs(b, fill=0x5A)
    if what == "null":
        outs["allele_map"] = None
    elif what == "site_begin":
        b["site_entry_begin"][1] = 5
    elif what == "allele_begin":
        b["entry_allele_begin"][2] = 1
    elif what == "gt_begin":
        b["entry_gt_begin"][1] = 7
    elif what == "blob":
        b["allele_off"][9] = b["blob_len"] - 4
    elif what == "gt":
        b["gt"][5] = -4
    elif what == "slot":
        b["out_allele_begin"][1] = 3
    elif what == "slot_decreases":
        b["out_allele_begin"][2] = 3
    return b, outs


ERRORS = [("null", "null field"), ("site_begin", "site_entry_begin decreases at site 1"), ("allele_begin", "entry_allele_begin decreases at entry 1"),
          ("gt_begin", "entry_gt_begin decreases at entry 1"), ("blob", "allele 9 .*ends beyond the blob"), ("gt", r"gt\[5\] is -4"),
          ("slot", "slot of site 0 holds 3 alleles, the site needs 4"), ("slot_decreases", "out_allele_begin decreases at site 1")]


@pytest.mark.parametrize("what,msg", ERRORS, ids=[w for w, _ in ERRORS])
def test_call_errors(what, msg):
    b, outs = broken(what)
    assert merge.call(b, outs, None, check=False) == -1   # TRGT_ERR_INVALID
    assert re.search(msg, _lib.lib().trgt_hip_last_error(None).decode())
    for a in outs.values():
        assert a is None or (a.view(np.uint8) == 0x5A).all()   # nothing written
    with pytest.raises(_lib.TrgtHipError, match=msg):
        merge.call(b, outs, None)


def test_vector_end_is_the_only_negative_value():
    b, outs = run_host([([[b"CAG", b"C"]], [[merge.VECTOR_END, 4, 1, 0]])])
    assert list(outs["gt_out"]) == [merge.VECTOR_END, 4, 1, 0] and int(outs["site_status"][0]) == 0
