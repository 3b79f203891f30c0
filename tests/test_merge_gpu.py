"""trgt_merge_exact_batch on the device against tests/pymerge.py, no tolerance: the designed cases per case and in one call, random sites,
the blob and the outputs on the host and in HBM, the statistics, the 4-bit hash of a developer context, and the call errors."""
import numpy as np
import pytest

import merge_cases
from trgt_amd import _lib, merge

pytestmark = pytest.mark.gpu

LIMIT = merge.site_alleles_limit()
DESIGNED = merge_cases.designed(LIMIT)
ALL = [s for _, s in DESIGNED]
MIXED = [x for i, s in enumerate(ALL) for x in ((s, ALL[20 + i % 6]) if i % 3 == 0 else (s,))]
RANDOM = merge_cases.RANDOM[:600]
SMALL = [s for s in ALL + RANDOM if sum(len(a) for a in s[0]) <= 64]   # a call whose largest site fits a wave


def run(ctx, sites, blob_dev=False, outs_dev=False, pad=merge_cases.PAD):
    import torch
    b = merge.pack(sites, pad=pad)
    outs = merge.alloc_outputs(b, fill=0x5A)
    blob = torch.from_numpy(b["allele_blob"]).cuda() if blob_dev else None
    dev = {k: torch.from_numpy(v).cuda() for k, v in outs.items()} if outs_dev else None
    merge.call(b, dev if outs_dev else outs, ctx, blob=blob)
    if outs_dev:
        torch.cuda.synchronize()
        outs = {k: v.cpu().numpy() for k, v in dev.items()}
    return b, outs


@pytest.fixture(scope="module")
def ctx():
    return _lib.context()


@pytest.mark.parametrize("name,site", DESIGNED, ids=[n for n, _ in DESIGNED])
def test_designed_case(ctx, name, site):
    b, outs = run(ctx, [site])
    merge_cases.check_outputs(b, outs, [site], name)
    n = sum(len(a) for a in site[0])
    assert ctx.merge_stats()[:2] == ((1, 0) if n <= LIMIT else (0, 1))


@pytest.mark.parametrize("blob_dev,outs_dev", [(False, False), (True, False), (False, True), (True, True)], ids=["host_host", "hbm_host", "host_hbm", "hbm_hbm"])
def test_all_designed_in_one_call(ctx, blob_dev, outs_dev):
    b, outs = run(ctx, MIXED, blob_dev, outs_dev)
    merge_cases.check_outputs(b, outs, MIXED, "mixed")
    stats = ctx.merge_stats()
    want = merge_cases.expected(MIXED)
    over = sum(1 for s in MIXED if sum(len(a) for a in s[0]) > LIMIT)
    assert over >= 1 and stats[1] == over and stats[0] == len(MIXED) - over          # the limit + 1 site takes the host route, nothing else does
    assert stats[2] == sum(1 for w in want if w[0] != 0) and stats[2] > 6
    assert stats[3] > 0


def test_random_sites(ctx):
    b, outs = run(ctx, RANDOM, blob_dev=True)
    merge_cases.check_outputs(b, outs, RANDOM, "random")


def test_one_wave_form(ctx):
    b, outs = run(ctx, SMALL)
    merge_cases.check_outputs(b, outs, SMALL, "small")
    b, outs = run(ctx, SMALL, pad=(0,))
    merge_cases.check_outputs(b, outs, SMALL, "small, packed")


def test_unaligned_device_blob(ctx):
    """the blob in HBM at an address that is no multiple of 4"""
    import torch
    sites = ALL[:20] + RANDOM[:100]
    b = merge.pack(sites, pad=merge_cases.PAD)
    outs = merge.alloc_outputs(b)
    for shift in (1, 2, 3):
        buf = torch.zeros(len(b["allele_blob"]) + 8, dtype=torch.uint8).cuda()
        buf[shift:shift + len(b["allele_blob"])] = torch.from_numpy(b["allele_blob"]).cuda()
        view = buf[shift:]
        assert view.data_ptr() % 4 == shift
        merge.call(b, outs, ctx, blob=view)
        merge_cases.check_outputs(b, outs, sites, "shift %d" % shift)


def test_four_bit_hash_changes_nothing_but_the_comparisons(ctx):
    sites = MIXED + RANDOM
    b, full = run(ctx, sites)
    full_stats = ctx.merge_stats()
    weak_ctx = _lib.context_with_env(TRGT_MERGE_HASH_BITS=4)
    try:
        b2, weak = run(weak_ctx, sites)
        weak_stats = weak_ctx.merge_stats()
    finally:
        weak_ctx.close()
    merge_cases.check_outputs(b2, weak, sites, "4-bit hash")
    want = merge_cases.expected(sites)
    slot = b["out_allele_begin"]
    for s, w in enumerate(want):   # identical arrays, wherever they are specified
        if w[0] == 0:
            e0, e1 = int(b["site_entry_begin"][s]), int(b["site_entry_begin"][s + 1])
            a0, a1 = int(b["entry_allele_begin"][e0]), int(b["entry_allele_begin"][e1])
            g0, g1 = int(b["entry_gt_begin"][e0]), int(b["entry_gt_begin"][e1])
            assert np.array_equal(full["allele_map"][a0:a1], weak["allele_map"][a0:a1]) and np.array_equal(full["gt_out"][g0:g1], weak["gt_out"][g0:g1])
            assert np.array_equal(full["out_allele_src"][int(slot[s]):int(slot[s]) + len(w[1])], weak["out_allele_src"][int(slot[s]):int(slot[s]) + len(w[1])])
    assert np.array_equal(full["site_status"], weak["site_status"]) and np.array_equal(full["out_n_alleles"], weak["out_n_alleles"])
    assert weak_stats[:3] == full_stats[:3]
    assert weak_stats[3] > full_stats[3] > 0, (weak_stats, full_stats)


def test_lane_and_wave_hash_forms_agree(ctx):
    """alleles hashed one per wave (TRGT_MERGE_LANE_MAX=0 on a developer context) and one per lane: the same results"""
    sites = ALL[:19] + RANDOM[:200]
    wave_ctx = _lib.context_with_env(TRGT_MERGE_LANE_MAX=0)
    try:
        b, outs = run(wave_ctx, sites)
    finally:
        wave_ctx.close()
    merge_cases.check_outputs(b, outs, sites, "one allele per wave")
    lane_ctx = _lib.context_with_env(TRGT_MERGE_LANE_MAX=1000000)
    try:
        b, outs = run(lane_ctx, sites)
    finally:
        lane_ctx.close()
    merge_cases.check_outputs(b, outs, sites, "one allele per lane")


def test_merge_exact_on_the_device(ctx):
    import pymerge
    site = DESIGNED[18][1]   # alt_equals_ref
    gts = [[[merge.gt_decode(v) for v in g]] for g in site[1]]
    assert merge.merge_exact(gts, site[0], ctx) == pymerge.merge_exact(gts, site[0])
    with pytest.raises(ValueError, match="^Reference alleles do not match: 'CAG' and 'CAT'$"):
        merge.merge_exact([[[]], [[]]], [[b"CAG"], [b"CAT"]], ctx)


def test_call_error_leaves_outputs_unwritten(ctx):
    import torch
    sites = ALL[:10]
    for outs_dev in (False, True):
        b = merge.pack(sites)
        b["gt"][3] = -7
        outs = merge.alloc_outputs(b, fill=0x5A)
        given = {k: torch.from_numpy(v).cuda() for k, v in outs.items()} if outs_dev else outs
        assert merge.call(b, given, ctx, check=False) == -1
        assert "gt[3] is -7" in _lib.lib().trgt_hip_last_error(ctx.handle).decode()
        for v in given.values():
            a = v.cpu().numpy() if outs_dev else v
            assert (a.view(np.uint8) == 0x5A).all()
    b = merge.pack(sites)
    b["out_allele_begin"][1:] -= 1
    outs = merge.alloc_outputs(b, fill=0x5A)
    assert merge.call(b, outs, ctx, check=False) == -1
    assert all((a.view(np.uint8) == 0x5A).all() for a in outs.values())


def test_kernel_times_only_when_timed(ctx):
    run(ctx, ALL[:10])
    assert merge.kernel_ms(ctx) == (0.0, 0.0)
    ctx.timing_enable(True)
    try:
        run(ctx, ALL[:10])
        h, s = merge.kernel_ms(ctx)
        assert h > 0 and s > 0
    finally:
        ctx.timing_enable(False)
