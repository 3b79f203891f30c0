"""trgt_merge_sites_host and trgt_amd.merge.merge_contig(ctx=None) without a GPU: every output array against tests/pymergesites.py on every
designed case and the random contigs, with no tolerance; the sizing protocol; the call errors; the loader's MERGE_SITES_EXPORTS against
the header."""
import os
import re

import numpy as np
import pytest

import merge_sites_cases as cases
import pymergesites as ps
from trgt_amd import _lib, merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESIGNED = cases.designed()
RANDOM = cases.random_contigs()
EXPECTED = {}


def expected(name, files):
    """the restatement's sites, computed once per case and left unchanged"""
    if name not in EXPECTED:
        EXPECTED[name] = ps.merge_variants(files)
    return EXPECTED[name]


def run(files, pad=(0,), ctx=None, fill=0x5A):
    b = merge.pack_sites(files, pad=pad)
    outs = merge.alloc_sites_outputs(b, len(ps.key_sites(files)), fill=fill)
    merge.call_sites(b, outs, len(ps.key_sites(files)), ctx)
    return b, outs


def test_exports_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trgt_hip_merge_sites.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(trgt_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.MERGE_SITES_EXPORTS)
    main_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trgt_hip.h")).read(), flags=re.S)
    assert main_h.index('extern "C"') < main_h.index('#include "trgt_hip_merge.h"') < main_h.index('#include "trgt_hip_merge_sites.h"')
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.MERGE_SITES_EXPORTS)
    assert not set(_lib.MERGE_SITES_EXPORTS) & set(_lib.EXPORTS + _lib.MERGE_EXPORTS)
    assert L.trgt_hip_abi_version() == 11


@pytest.mark.parametrize("name,files,pad", DESIGNED, ids=[n for n, _, _ in DESIGNED])
def test_designed_case(name, files, pad):
    for p in ((0,), pad):
        b, outs = run(files, pad=p)
        cases.check_outputs(files, b, outs, expected(name, files), name)


def test_random_contigs():
    n_ragged = n_padded = n_dup = 0
    for k, files in enumerate(RANDOM):
        exp = expected("random%d" % k, files)
        b, outs = run(files, pad=(0, 3, 1))
        cases.check_outputs(files, b, outs, exp, "random%d" % k)
        n_ragged += sum(e["status"] == ps.RAGGED for e in exp)
        n_padded += sum(len(e["padded"] or []) for e in exp)
        n_dup += len(exp) - len({e["pos"] for e in exp})
    assert n_ragged > 10 and n_padded > 100 and n_dup > 20


def test_merge_contig_equals_the_restatement():
    for name, files, _ in DESIGNED:
        cases.check_contig(files, merge.merge_contig(files), expected(name, files), name)
    for k, files in enumerate(RANDOM[:60]):
        cases.check_contig(files, merge.merge_contig(files), expected("random%d" % k, files), "random%d" % k)


def test_sites_batch_lists_the_sites():
    name, files, _ = next(c for c in DESIGNED if c[0] == "three_and_four_records_at_one_position")
    got = merge.sites_batch(files)
    assert [(s["pos"], s["records"]) for s in got] == [(7, [0, 4, 5, 9]), (7, [1, -1, 6, -1]), (7, [2, -1, 7, -1]), (7, [-1, -1, 8, -1]), (9, [3, -1, -1, 10])]
    assert [s["template"] for s in got] == [0, 1, 2, 8, 3]
    assert merge.sites_batch([]) == [] and merge.merge_contig([dict(n_samples=2, pre_v1=True, am_is_int=False, records=[])]) == []


def sizing_protocol(ctx):
    name, files, _ = next(c for c in DESIGNED if c[0] == "samples_1_2_3")
    b = merge.pack_sites(files)
    n = len(expected(name, files))
    probe = dict(record_site=np.full(b["n_records"], -7, np.int32))
    assert merge.call_sites(b, probe, 0, ctx, check=False) == merge.ERR_NOMEM and probe["n_sites"] == n
    want_site = probe["record_site"].copy()
    assert (want_site >= 0).all()
    outs = merge.alloc_sites_outputs(b, n - 1, fill=0xC3)     # one site short: nothing but n_sites and record_site
    canary = {k: v.copy() for k, v in outs.items()}
    assert merge.call_sites(b, outs, n - 1, ctx, check=False) == merge.ERR_NOMEM and outs["n_sites"] == n
    assert "sites" in _lib.lib().trgt_hip_last_error(ctx.handle if ctx else None).decode()
    for k, v in canary.items():
        assert (outs[k] == (want_site if k == "record_site" else v)).all(), k
    outs = merge.alloc_sites_outputs(b, n, fill=0xC3)         # exactly n_sites
    merge.call_sites(b, outs, n, ctx)
    cases.check_outputs(files, b, outs, expected(name, files), name)
    outs = merge.alloc_sites_outputs(b, n + 3, fill=0xC3)     # more room than sites: the rest stays untouched
    merge.call_sites(b, outs, n + 3, ctx)
    cases.check_outputs(files, b, outs, expected(name, files), name)
    assert (outs["site_pos"][n:].view(np.uint8) == 0xC3).all() and (outs["al"][n * b["S"] * 2:].view(np.uint8) == 0xC3).all()


def test_sizing_protocol():
    sizing_protocol(None)


def broken_calls():
    """[(what, the word the message must carry, the code, a function that breaks a packed input / its outputs / cap)]"""
    def field(k, key, i, v):
        def f(b, outs):
            b[k][key] = b[k][key].copy()
            b[k][key][i] = v
        return f

    def arr(key, i, v):
        def f(b, outs):
            b[key] = b[key].copy()
            b[key][i] = v
        return f

    def drop_in(key):
        def f(b, outs):
            b[key] = None
        return f

    def drop_out(key):
        def f(b, outs):
            outs[key] = None
        return f

    def small_blob(b, outs):
        outs["allele_blob"] = outs["allele_blob"][:8]
    I, U = merge.ERR_INVALID, merge.ERR_UNSUPPORTED
    return [("null pos", "pos", I, drop_in("pos")), ("null n_samples", "n_samples", I, drop_in("n_samples")), ("null out gt", "gt", I, drop_out("gt")),
            ("null record_site", "record_site", I, drop_out("record_site")), ("null allele_len", "allele_len", I, drop_in("allele_len")),
            ("file_record_begin start", "file_record_begin", I, arr("file_record_begin", 0, 1)), ("file_record_begin decreases", "decreases", I, arr("file_record_begin", 1, 99)),
            ("record_allele_begin decreases", "record_allele_begin", I, arr("record_allele_begin", 1, 50)), ("n_samples 0", "n_samples", I, arr("n_samples", 1, 0)),
            ("sd begin start", "sd.begin", I, field("SD", "begin", 0, 1)), ("ap begin disagrees", "n_samples * width", I, field("AP", "begin", 2, 1000)),
            ("al begin decreases", "al.begin", I, field("AL", "begin", 2, 0)), ("gt width 0", "gt.width", I, field("gt", "width", 1, 0)),
            ("am width 3", "am.width", U, field("AM", "width", 1, 3)), ("pos decreases", "decreases", I, arr("pos", 1, 0)), ("pos negative", "outside", I, arr("pos", 0, -1)),
            ("pos 2^40", "outside", I, arr("pos", 3, 1 << 40)), ("allele beyond the blob", "beyond the blob", I, arr("allele_len", 2, 1 << 20)),
            ("blob_cap too small", "blob_cap", I, small_blob)]


def call_errors(ctx, with_the_large_one=True):
    files = [cases.make_file(cases.random.Random(5), [10, 20, 20, 30], 2, pre_v1=True), cases.make_file(cases.random.Random(6), [20, 40], 1, am_is_int=True)]
    for what, word, code, breaker in broken_calls():
        b = merge.pack_sites(files)
        outs = merge.alloc_sites_outputs(b, 8, fill=0x3C)
        canary = {k: v.copy() for k, v in outs.items()}
        breaker(b, outs)
        rc = merge.call_sites(b, outs, 8, ctx, check=False)
        msg = _lib.lib().trgt_hip_last_error(ctx.handle if ctx else None).decode()
        assert rc == code and word in msg and ("trgt_merge_sites_batch" if ctx else "trgt_merge_sites_host") in msg, (what, rc, msg)
        assert "TRGT_" not in msg, msg
        for k, v in canary.items():
            if outs[k] is not None:
                assert (outs[k] == v[:len(outs[k])]).all(), (what, k)
    if not with_the_large_one:
        return
    # more than 2^24 - 1 records of one file at one position
    n = (1 << 24) + 1
    one = lambda t, v=0: np.full(n, v, t)  # noqa: E731
    ramp = np.arange(n + 1, dtype=np.uint64)
    b = dict(n_files=1, n_samples=np.array([1], np.int32), pre_v1=np.zeros(1, np.uint8), am_is_int=np.zeros(1, np.uint8), file_record_begin=np.array([0, n], np.uint64),
             pos=one(np.int64, 5), pad_base=one(np.uint8), record_allele_begin=np.zeros(n + 1, np.uint64), allele_off=np.zeros(1, np.uint64), allele_len=np.zeros(1, np.uint32),
             allele_blob=np.zeros(1, np.uint8), blob_len=0, n_records=n, n_alleles=0, S=1, any_pre_v1=False, blob_need=0)
    width, values = one(np.uint8, 1), one(np.uint32)
    for k in merge.FIELDS:
        b[k] = dict(width=width, begin=ramp, values=values)
    probe = dict(record_site=one(np.int32, -7))
    assert merge.call_sites(b, probe, 0, ctx, check=False) == merge.ERR_UNSUPPORTED
    assert "2^24 - 1 records" in _lib.lib().trgt_hip_last_error(ctx.handle if ctx else None).decode() and (probe["record_site"] == -7).all()


def test_call_errors():
    call_errors(None)
