"""trgt_merge_sites_batch on the device against tests/pymergesites.py, no tolerance: the designed cases per case and in one call, the
random contigs, the blobs and the rows on the host and in HBM (a device blob at an odd address among them), merge_contig chained into
trgt_merge_exact_batch with the blob staying in HBM, the statistics, the sizing protocol and the call errors."""
import numpy as np
import pytest

import merge_sites_cases as cases
import pymergesites as ps
import test_merge_sites_host as host
from trgt_amd import _lib, merge

pytestmark = pytest.mark.gpu

DESIGNED = host.DESIGNED
RANDOM = host.RANDOM
expected = host.expected


@pytest.fixture(scope="module")
def ctx():
    return _lib.context()


def run(ctx, files, pad=(0,), blob_dev=False, rows_dev=False, blob_shift=0, cap_extra=0):
    """one call; blob_dev: the input blob and the output blob in HBM, both blob_shift bytes behind an aligned address"""
    import torch
    b = merge.pack_sites(files, pad=pad)
    n = len(ps.key_sites(files)) + cap_extra
    outs = merge.alloc_sites_outputs(b, n, fill=0x5A)
    blob, dev = None, {}
    if blob_dev:
        blob = torch.zeros(b["allele_blob"].size + 8, dtype=torch.uint8, device="cuda")[blob_shift:blob_shift + b["allele_blob"].size]   # the input blob behind the same shift
        blob.copy_(torch.from_numpy(b["allele_blob"]))
        dev["allele_blob"] = torch.full((outs["allele_blob"].size + 8,), 0x5A, dtype=torch.uint8, device="cuda")[blob_shift:blob_shift + outs["allele_blob"].size]
    if rows_dev:
        for k in ("al", "sd", "ap", "am", "sample_src"):
            dev[k] = torch.from_numpy(outs[k].view(np.int32)).cuda()
    outs.update(dev)
    merge.call_sites(b, outs, n, ctx, blob=blob)
    if dev:
        torch.cuda.synchronize()
        for k in dev:
            outs[k] = outs[k].cpu().numpy().view(dict(merge.SITES_OUT)[k])
    return b, outs


@pytest.mark.parametrize("name,files,pad", DESIGNED, ids=[n for n, _, _ in DESIGNED])
def test_designed_case(ctx, name, files, pad):
    exp = expected(name, files)
    b, outs = run(ctx, files, pad=pad)
    cases.check_outputs(files, b, outs, exp, name)
    stats = ctx.merge_sites_stats()
    assert stats[:2] == (len(exp), sum(e["status"] == ps.RAGGED for e in exp))
    if not any(e["status"] == ps.RAGGED for e in exp):
        assert stats[2] == sum(len(e["padded"]) for e in exp)
    assert stats[3] == outs["blob_written"]


def shifted(files, by):
    return [dict(f, records=[dict(r, pos=r["pos"] + by) for r in f["records"]]) for f in files]


def all_in_one():
    """every designed case with a file count of up to 65, side by side in one contig: the files of all cases, each case at positions of its own"""
    files, names = [], []
    fits = [c for c in DESIGNED if len(c[1]) <= 65 and all(r["pos"] < (1 << 20) for f in c[1] for r in f["records"])]   # (the rest: cases of their own)
    for k, (name, f, _) in enumerate(fits):
        files.extend(shifted(f, k << 20))
        names.append(name)
    return files, names


@pytest.mark.parametrize("blob_dev,rows_dev,shift", [(False, False, 0), (True, False, 0), (False, True, 0), (True, True, 1), (True, True, 3)],
                         ids=["host_host", "hbm_host", "host_hbm", "hbm_hbm_odd", "hbm_hbm_3"])
def test_all_designed_in_one_call(ctx, blob_dev, rows_dev, shift):
    files, names = all_in_one()
    assert len(names) >= 25 and len(files) > 256
    exp = expected("all_in_one", files)
    b, outs = run(ctx, files, pad=(0, 1, 2, 3, 1), blob_dev=blob_dev, rows_dev=rows_dev, blob_shift=shift)
    cases.check_outputs(files, b, outs, exp, "all_in_one")
    stats = ctx.merge_sites_stats()
    assert stats[0] == len(exp) and stats[1] == sum(e["status"] == ps.RAGGED for e in exp) and stats[1] >= 11
    assert stats[2] > 100 and stats[3] == outs["blob_written"] > 0


def test_random_contigs(ctx):
    for k, files in enumerate(RANDOM):
        b, outs = run(ctx, files, pad=(0, 3, 1), blob_dev=k % 3 == 0, rows_dev=k % 2 == 0, blob_shift=k % 4)
        cases.check_outputs(files, b, outs, expected("random%d" % k, files), "random%d" % k)


def test_merge_contig_on_a_context_equals_the_restatement(ctx):
    for name, files, _ in DESIGNED:
        cases.check_contig(files, merge.merge_contig(files, ctx), expected(name, files), name)
    for k, files in enumerate(RANDOM[:40]):
        cases.check_contig(files, merge.merge_contig(files, ctx), expected("random%d" % k, files), "random%d" % k)


def test_the_output_blob_goes_to_merge_exact_without_leaving_hbm(ctx):
    import torch
    name, files, pad = next(c for c in DESIGNED if c[0] == "allele_lengths_pre_v1_some")
    b = merge.pack_sites(files, pad=pad)
    outs = merge.run_sites(b, ctx, device_outputs=True)
    assert isinstance(outs["allele_blob"], torch.Tensor) and outs["allele_blob"].is_cuda and outs["blob_written"] > 0
    b2, dev_blob = merge.merge_in_of_sites(b, outs)
    assert dev_blob is outs["allele_blob"] and b2["allele_blob"] is None
    outs2 = merge.alloc_outputs(b2)
    merge.call(b2, outs2, ctx, blob=dev_blob)
    exp = expected(name, files)
    assert [int(v) for v in outs2["site_status"][:len(exp)]] == [e["status"] for e in exp]
    assert [int(v) for v in outs2["out_n_alleles"][:len(exp)]] == [len(e["alleles"]) if e["status"] == 0 else 0 for e in exp]
    assert sum(e["status"] == 0 for e in exp) >= 30


def test_timing_has_three_kernel_groups(ctx):
    name, files, pad = next(c for c in DESIGNED if c[0] == "allele_lengths_pre_v1_all")
    ctx.timing_enable(True)
    try:
        run(ctx, files)
        ms = merge.sites_kernel_ms(ctx)
    finally:
        ctx.timing_enable(False)
    assert len(ms) == 3 and all(v > 0 for v in ms)
    run(ctx, files)
    assert merge.sites_kernel_ms(ctx) == (0.0, 0.0, 0.0)


def test_sizing_protocol(ctx):
    host.sizing_protocol(ctx)


def test_call_errors(ctx):
    host.call_errors(ctx, with_the_large_one=False)
