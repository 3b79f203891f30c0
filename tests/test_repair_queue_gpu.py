"""The queue in front of a consensus repair (trgt_amd/csrc/repair_queue.hpp) when the arenas run out: TRGT_REPAIR_ARENA_KB caps the CIGAR,
result and vote-scratch arenas of the size and haplotype-tag routes, as TRGT_CLUSTER_ARENA_KB does for the cluster chains.  A locus that
finds no room is refused before it takes a job, a group or a place in the list of waiting loci, and takes the host path: same results.
One switch caps all three arenas in the proportion of their natural sizes, and with these cases the CIGAR arena is always the first to run
out: what is exercised is the refusal at the first arena.  The early stops behind it (result arena full, scratch full after the other
two were taken) would need a cap per arena and are not reached by any test.

The caps are worked out on the CPU from the oracle's kept reads and group_needs as test_repair_needs.py restates it.  Of a size-route locus
the oracle reports how many consensus alignments it ran (the members of its vote groups, unique sequences of the kept reads) but not the
groups, so its need is bounded, not restated: below with the shortest, above with the longest unique sequences as members and backbone."""
import pytest

import flank_deep_cases as fc
import test_flank_deep_gpu as fdg
import test_flank_device_gpu as fg
import test_size_deep_gpu as sdg
from test_locus_gpu import _oracle_locus
from test_repair_needs import group_needs

pytestmark = pytest.mark.gpu
WORDS_PER_KB, NO_ROOM_KB = 256, 1  # the CIGAR and scratch arenas are counted in words, the result arena in bytes


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def noisy(oracle, locus):
    """the 60-locus batch of test_locus_batch_noisy_reads_trigger_consensus_repair, the oracle's result of every locus, and per locus that
    aligns for a repair (alignments, lower bound, upper bound of its needs as group_needs returns them)"""
    from trgt_amd import synth
    b = synth.generate(60, first_locus=5000, sub_rate=0.004, ins_rate=0.004, del_rate=0.004, stutter_rate=0.3)
    refs = [_oracle_locus(oracle, b, l, locus.Params()) for l in range(60)]
    return b, refs, [_size_route_bounds(b, ref, l) for l, ref in enumerate(refs) if ref["stats"]["n_wfa_cons"] > 0]


def _size_route_bounds(b, ref, l):
    a0, nc = int(b["locus_read_begin"][l]), int(ref["stats"]["n_wfa_cons"])
    off = [int(b["read_off"][a0 + int(k)]) for k in ref["kept_read"]]
    uniq = sorted(len(s) for s in set(bytes(b["read_blob"][o + int(ref["span_start"][int(k)]):o + int(ref["span_end"][int(k)])]) for o, k in zip(off, ref["kept_read"])))
    assert 0 < nc <= len(uniq)
    # the CIGAR words do not depend on how the members split into groups; of everything else two groups take one more backbone than one
    lo, hi, top = uniq[0], uniq[-1], sum(uniq[-nc:])
    lower = group_needs(lo, nc, sum(uniq[:nc]))
    upper = (nc * (hi + 1) + top, None, 2 * (hi + 16 + 15) + top, 2 * group_needs(hi, 0, 0)[3] + 3 * nc)
    return nc, lower, upper


def _tag_route_cigar_words(L, q):
    """CIGAR words of a locus on the tag route, at least: every read of a group below 50 % is a member, the backbone is one of them"""
    route = fc.on_route(L, q, fc.CEILING)
    assert route is not None and route[1]
    words = 0
    for g in (0, 1):
        lens = [len(s) for s, a in zip(fc.kept_segments(L, q), route[0]) if a == g]
        if max(fc.group_counts(L, q, route[0], g).values()) / len(lens) < 0.5:
            words += group_needs(min(lens), len(lens), sum(lens))[0]
    return words


def test_no_room_size_route(oracle, locus, noisy):
    from trgt_amd import _lib
    b, refs, needs = noisy
    assert len(needs) > 5 and all(lower[0] > NO_ROOM_KB * WORDS_PER_KB for _, lower, _ in needs), min(lower[0] for _, lower, _ in needs)
    ctx = _lib.context_with_env(TRGT_REPAIR_ARENA_KB=NO_ROOM_KB)
    try:
        out = locus.run_batch(b, ctx=ctx)
        sdg._compare(locus, b, out, refs)
        print("no room, size route: stats[18:21]", out.stats[18:21], "repair loci", len(needs))
        assert int(out.stats[18]) == 0 and int(out.stats[19]) == len(needs) and int(out.stats[20]) == 0
    finally:
        ctx.close()


def test_no_room_tag_route(oracle, locus):
    from trgt_amd import _lib
    loci = fg.case_repair()
    plain = [fg._ref(oracle, L, locus.Params(), meta=False) for L in loci]
    assert all(_tag_route_cigar_words(L, q) > NO_ROOM_KB * WORDS_PER_KB for L, q in zip(loci, plain))
    ctx = _lib.context_with_env(TRGT_REPAIR_ARENA_KB=NO_ROOM_KB)
    try:
        ctx.set_flank_device(True)
        b, _, _ = fg._check(oracle, locus, None, loci, handed=(0, 1, 2), want=(0, 0, 3, 0), on_ctx=ctx)  # handed, not done
        out = locus.run_batch(b, ctx=ctx)
        assert int(out.stats[18]) == 0 and int(out.stats[19]) == 3, out.stats[18:21]
    finally:
        ctx.close()


def test_no_room_deep_size_route(oracle, locus):
    from trgt_amd import _lib
    mk = sdg.Maker(202)  # case 2 of test_size_deep_gpu.py
    loci, params = [mk.het(300, 0.03), mk.het(600, 0.03)], locus.Params(**sdg.DEEP)
    ctx = _lib.context_with_env(TRGT_REPAIR_ARENA_KB=NO_ROOM_KB)
    try:
        ctx.set_size_max_reads(_lib.size_max_reads_limit())
        b, refs = sdg._check(oracle, locus, loci, params, ctx, (0, 0, 2))  # both handed to the host path
        assert sdg._repaired(b, refs) == 2 and all(_size_route_bounds(b, ref, l)[1][0] > NO_ROOM_KB * WORDS_PER_KB for l, ref in enumerate(refs))
        out = locus.run_batch(b, params, ctx=ctx)
        assert int(out.stats[18]) == 0 and int(out.stats[19]) == 2, out.stats[18:21]
    finally:
        ctx.close()


def test_no_room_deep_tag_route(oracle, locus):
    from trgt_amd import _lib
    loci, params = fc.case_repair(), locus.Params(**fc.DEEP)
    _, plain = fc.oracle_pair(oracle, loci, params)
    assert all(_tag_route_cigar_words(L, q) > NO_ROOM_KB * WORDS_PER_KB for L, q in zip(loci, plain))
    ctx = _lib.context_with_env(TRGT_REPAIR_ARENA_KB=NO_ROOM_KB)
    try:
        ctx.set_flank_device(True); ctx.set_size_max_reads(_lib.size_max_reads_limit())
        b, _, _ = fdg._check(oracle, locus, None, loci, fc.DEEP, handed=(0, 1, 2), want=((0, 0, 3, 0), (0, 0, 3, 0)), both_ctx=ctx)
        out = locus.run_batch(b, params, ctx=ctx)
        assert int(out.stats[18]) == 0 and int(out.stats[19]) == 3, out.stats[18:21]
    finally:
        ctx.close()


def test_room_for_some(oracle, locus, noisy):
    """A cap that takes the largest locus alone but not all of them.  A refused reservation is not rolled back and the workgroups race, so
    which loci fit differs from run to run; asserted is what holds in every order: the first locus to reserve fits, not all can, every
    result is the oracle's, and the alignments the device did not run are those of as many loci as were refused.  The outputs carry no
    per-locus mark of the path a locus took, so the check cannot name the refused loci: it accepts any set of that many repair loci whose
    alignments add up to the difference."""
    from trgt_amd import _lib
    b, refs, needs = noisy
    fits_one = max(max(-(-u[0] // WORDS_PER_KB), -(-u[2] // 1024), -(-u[3] // WORDS_PER_KB)) for _, _, u in needs)  # KB that hold any one locus
    holds_all = sum(lower[0] for _, lower, _ in needs) // WORDS_PER_KB  # KB whose CIGAR words all loci together exceed
    kb = (fits_one + holds_all) // 2
    print("room for some: KB", fits_one, "<=", kb, "<", holds_all)
    assert fits_one <= kb and kb * WORDS_PER_KB < sum(lower[0] for _, lower, _ in needs)
    total = sum(nc for nc, _, _ in needs)
    sums = {(0, 0)}  # (loci, alignments) of every set of repair loci
    for nc, _, _ in needs:
        sums |= {(c + 1, s + nc) for c, s in sums}
    ctx = _lib.context_with_env(TRGT_REPAIR_ARENA_KB=kb)
    try:
        out = locus.run_batch(b, ctx=ctx)
        sdg._compare(locus, b, out, refs)
        done, refused, on_device, aligned = (int(out.stats[i]) for i in (18, 19, 20, 1))
        print("room for some: loci repaired", done, "refused", refused, "alignments on the device", on_device, "of", aligned)
        assert done >= 1 and refused >= 1 and done + refused == len(needs)
        assert aligned == total and (refused, aligned - on_device) in sums
    finally:
        ctx.close()
