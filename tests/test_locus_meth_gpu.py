"""trgt_locus_meth_batch on the GPU, through the C ABI: every designed case of tests/meth_cases.py against tests/pymeth.py bit for bit, both
read encodings, host and device blobs, the two error classes, and one end-to-end leg behind the real trgt_locus_batch."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meth_cases  # noqa: E402
import pymeth  # noqa: E402

pytestmark = pytest.mark.gpu

IN_KEYS = ("locus_read_begin", "read_blob", "read_off", "read_len")
OUT_KEYS = ("span_start", "span_end", "read_rank", "n_alleles", "ci", "allele_len", "gt_size", "flipped")


@pytest.fixture(scope="module")
def ctx():
    from trgt_amd import _lib
    return _lib.context()


def call(ctx, a, reads_dev=None, meth_dev=None, want_reads=True, want_read_meth=True, **replace):
    """trgt_locus_meth_batch on the arrays of meth_cases.build().  reads_dev / meth_dev: device tensors to pass instead of the host blobs;
    replace: arrays to pass instead of a's (None: a NULL pointer).  Returns (rc, message, allele_meth, meth_reads, read_meth)."""
    from trgt_amd import _lib
    a = dict(a, **replace)
    p = lambda v: None if v is None else _lib.ptr(v).value
    cin, cout = _lib.LocusBatchIn(), _lib.LocusBatchOut()
    cin.n_loci, cin.read_encoding = int(a["n_loci"]), int(a["read_encoding"])
    for k in IN_KEYS:
        setattr(cin, k, p(reads_dev if k == "read_blob" and reads_dev is not None else a[k]))
    for k in OUT_KEYS:
        setattr(cout, k, p(a[k]))
    nl, nr = int(a["n_loci"]), int(a["n_reads"])
    am, n, rm = np.full(2 * nl + 2, 7.0), np.full(2 * nl + 2, 7, np.int32), np.full(nr + 2, 7.0)   # (two spare slots each: nothing may be written there)
    rc = _lib.lib().trgt_locus_meth_batch(ctx.handle, C.addressof(cin), C.addressof(cout), p(meth_dev if meth_dev is not None else a["meth"]), p(a["meth_off"]),
                                          p(a["has_meth"]), p(am), p(n) if want_reads else None, p(rm) if want_read_meth else None)
    msg = _lib.lib().trgt_hip_last_error(ctx.handle).decode() if rc else ""
    assert (am[2 * nl:] == 7.0).all() and (n[2 * nl:] == 7).all() and (rm[nr:] == 7.0).all()
    return rc, msg, am[:2 * nl], n[:2 * nl], rm[:nr]


def same_bits(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all(), (got, want)
    ok = ~np.isnan(want)
    assert (got[ok].view(np.uint64) == want[ok].view(np.uint64)).all(), (got, want)


GOOD = [k for k, (_, notes) in meth_cases.CASES.items() if "error" not in notes]


@pytest.mark.parametrize("name", GOOD)
def test_designed_case(ctx, name):
    loci, notes = meth_cases.CASES[name]
    null = notes.get("gt_size_null", False)
    am, n, rm = meth_cases.expected(loci, gt_size_null=null)
    for encoding in (0, 1):
        for lead in (0, 1, 2, 3):   # every alignment of the blob's first read (and, with it, other ones for the rest)
            a = meth_cases.build(loci, encoding, lead, null)
            rc, msg, g_am, g_n, g_rm = call(ctx, a)
            assert rc == 0, msg
            same_bits(g_am, am)
            same_bits(g_rm, rm)
            assert (g_n == n).all(), (encoding, lead, g_n, n)
    # the optional outputs left out
    rc, msg, g_am, _, _ = call(ctx, meth_cases.build(loci, 0, 0, null), want_reads=False, want_read_meth=False)
    assert rc == 0, msg
    same_bits(g_am, am)


def test_host_and_device_blobs_give_the_same_bits(ctx):
    import torch
    loci, _ = meth_cases.CASES["mixed"]
    am, n, rm = meth_cases.expected(loci)
    for encoding in (0, 1):
        a = meth_cases.build(loci, encoding, 1)
        # the device blobs at an odd address inside their allocations: nothing may rest on hipMalloc's alignment
        rt, mt = torch.zeros(len(a["read_blob"]) + 8, dtype=torch.uint8, device="cuda"), torch.zeros(len(a["meth"]) + 8, dtype=torch.uint8, device="cuda")
        rt[3:3 + len(a["read_blob"])] = torch.from_numpy(a["read_blob"]).cuda()
        mt[5:5 + len(a["meth"])] = torch.from_numpy(a["meth"]).cuda()
        for reads, meth in ((None, None), (rt[3:], None), (None, mt[5:]), (rt[3:], mt[5:])):
            rc, msg, g_am, g_n, g_rm = call(ctx, a, reads_dev=reads, meth_dev=meth)
            assert rc == 0, msg
            same_bits(g_am, am)
            same_bits(g_rm, rm)
            assert (g_n == n).all()


def test_malformed_profile_is_an_error_that_names_the_read(ctx):
    loci, notes = meth_cases.CASES["malformed_in_span"]
    for encoding in (0, 1):
        rc, msg, *_ = call(ctx, meth_cases.build(loci, encoding))
        assert rc == -1 and "read %d has malformed methylation profile" % notes["error"][1] in msg, msg
    # the context stays usable
    rc, msg, g_am, _, _ = call(ctx, meth_cases.build(meth_cases.CASES["anchor"][0]))
    assert rc == 0 and g_am[0] == 0.1


def test_invalid_input_is_refused_before_any_launch(ctx):
    from trgt_amd import _lib
    loci, _ = meth_cases.CASES["two_alleles"]
    a = meth_cases.build(loci)
    ctx.timing_enable(True)
    try:
        assert call(ctx, a)[0] == 0
        ms = (C.c_double * 2)()
        _lib.lib().trgt_locus_meth_kernel_ms(ctx.handle, ms)
        before = (ms[0], ms[1])
        assert before[0] > 0 and before[1] > 0
        bad = []
        for s0, s1 in ((-1, 5), (6, 5), (0, int(a["read_len"][0]) + 1)):
            ss, se = a["span_start"].copy(), a["span_end"].copy()
            ss[0], se[0] = s0, s1
            bad.append((dict(span_start=ss, span_end=se), "span"))
        mo = a["meth_off"].copy()
        mo[1] = mo[2] + 1
        bad.append((dict(meth_off=mo), "meth_off decreases"))
        rk = a["read_rank"].copy()
        rk[1] = rk[0]
        bad.append((dict(read_rank=rk), "rank"))
        rk = a["read_rank"].copy()
        rk[0] = 99
        bad.append((dict(read_rank=rk), "rank"))
        for k in ("read_blob", "read_off", "read_len", "locus_read_begin", "span_start", "span_end", "read_rank", "n_alleles", "ci", "allele_len", "meth", "meth_off", "has_meth"):
            bad.append(({k: None}, "null"))
        bad.append((dict(read_encoding=2), "read_encoding"))
        for replace, word in bad:
            rc, msg, *_ = call(ctx, a, **replace)
            assert rc == -1 and word in msg, (replace.keys(), msg)
            # no kernel of the call ran: the timed kernels are still the earlier call's
            _lib.lib().trgt_locus_meth_kernel_ms(ctx.handle, ms)
            assert (ms[0], ms[1]) == before
        # an unkept read may carry any span
        ss = a["span_start"].copy()
        rk = a["read_rank"].copy()
        ss[4], rk[4] = -5, -1
        assert call(ctx, a, span_start=ss, read_rank=rk)[0] == 0
    finally:
        ctx.timing_enable(False)


def _loci_of(b):
    """the loci of a synthetic batch as pack()'s dicts"""
    loci = []
    for l in range(int(b["n_loci"])):
        a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        m0, m1 = int(b["set_motif_begin"][l]), int(b["set_motif_begin"][l + 1])
        cut = lambda blob, o, n: bytes(blob[int(o):int(o) + int(n)])
        loci.append(dict(left_flank=cut(b["flank_blob"], b["lf_off"][l], b["lf_len"][l]), right_flank=cut(b["flank_blob"], b["rf_off"][l], b["rf_len"][l]),
                         tr=cut(b["tr_blob"], b["tr_off"][l], b["tr_len"][l]), ploidy=int(b["ploidy"][l]), genotyper=int(b["genotyper"][l]),
                         motifs=[cut(b["motif_blob"], b["motif_off"][m], int(b["motif_off"][m + 1]) - int(b["motif_off"][m])) for m in range(m0, m1)],
                         reads=[cut(b["read_blob"], b["read_off"][r], b["read_len"][r]) for r in range(a0, a1)]))
    return loci


def test_end_to_end_behind_trgt_locus_batch(ctx):
    """Synthetic cfg2 and cfg5 loci through the real trgt_locus_batch, random calls on most reads: analyze_batch's Allele.meth is pymeth
    applied to the GPU's own spans, ranks, genotype sizes and swap flags."""
    from trgt_amd import locus, synth
    loci = _loci_of(synth.generate(40, first_locus=7)) + _loci_of(synth.generate(10, first_locus=3, config=5))
    rng = random.Random(20250509)
    for L in loci:
        L["meth"] = [None if rng.random() < 0.15 else (b"" if rng.random() < 0.05 else meth_cases.calls_for(rng, r)) for r in L["reads"]]
    batch = locus.pack(loci)
    out = locus.run_batch(batch, ctx=ctx)
    assert out.gt_size.any() and (out.n_alleles > 0).sum() >= 40
    want, want_n = [], []
    for l, L in enumerate(loci):
        a0, a1 = int(batch["locus_read_begin"][l]), int(batch["locus_read_begin"][l + 1])
        am, n, _ = pymeth.locus_meth(int(out.n_alleles[l]), [int(v) for v in out.gt_size[2 * l:2 * l + 2]], [int(v) for v in out.ci[4 * l:4 * l + 4]], int(out.flipped[l]),
                                     list(zip(L["reads"], L["meth"])), [(int(out.span_start[r]), int(out.span_end[r])) for r in range(a0, a1)],
                                     [int(out.read_rank[r]) for r in range(a0, a1)])
        want += am; want_n += n
    g_am, g_n, _ = locus.allele_meth(batch, out, ctx)
    same_bits(g_am, want)
    assert list(g_n) == want_n
    # (the leg is not empty: 6 of the 40 cfg2 motifs and all 10 cfg5 motif sets hold a CpG, and their alleles average several reads)
    assert np.isfinite(g_am).sum() >= 12 and (np.asarray(want_n) > 1).sum() >= 8
    res = locus.analyze_batch(loci, ctx=ctx)
    got = [a.meth for r in res for a in r.genotype]
    exp = [None if v != v else v for l in range(len(loci)) for v in want[2 * l:2 * l + int(out.n_alleles[l])]]
    assert got == exp
    # chunks of the batch carry the calls with them (driver.split_batch), and the 4-bit form of the reads gives the same bits
    from trgt_amd import driver
    for chunk, lo in zip(driver.split_batch(batch, 16), range(0, len(loci), 16)):
        o = locus.run_batch(chunk, ctx=ctx)
        same_bits(locus.allele_meth(chunk, o, ctx)[0], want[2 * lo:2 * (lo + int(chunk["n_loci"]))])
    same_bits(locus.allele_meth(locus.pack_bam4(batch), out, ctx)[0], want)
