"""consensus_vote_kernel (trgt_amd/csrc/consensus_vote.hpp: repair_consensus, consensus.rs:5-111, on the device) against the restatement
written from the reference alone (tests/pyconsensus.py), on the hand-built groups of tests/consensus_cases.py.

Two routes reach the kernel.  The developer build's trgt_dev_consensus_vote takes groups and CIGARs as given and launches through the
same vote_groups that consensus_repair_batch uses, in both launch forms (count on the host: the host routes; count read from device
memory under a larger grid: the device chains): that is the developer library's copy of the kernel.  The release library's copy is
reached with haploid cluster-genotyper loci whose every voting segment the test chooses (ploidy 1, Genotyper::Cluster: the genotype is
one make_consensus over all kept reads), on the one-wave chain, the host cluster path and the deep chain; there the CIGARs are BiWFA's,
computed again through WFAligner for the expectation.  tests/test_consensus_cases.py ties the oracle to the same restatement without a
GPU and asserts that the random lists reach the decisions they are meant to reach."""
import ctypes as C

import numpy as np
import pytest

import consensus_cases as cases
import pyconsensus

pytestmark = pytest.mark.gpu

NO_FIT = 0xFFFFFFFF


def _lib_mod():
    from trgt_amd import _lib
    return _lib


def restate(backbone, members):
    return pyconsensus.repair_consensus(backbone, [m for m, _ in members], [ops for _, ops in members])


@pytest.fixture(scope="module")
def dev_ctx():
    """a context of the developer library, and that library"""
    _lib = _lib_mod()
    _lib.lib()  # (binds the HIP runtime that torch brought, as every other test does, before the developer library loads)
    L = _lib.dev_lib()
    assert L is not None, "trgt_amd/libtrgt_hip_dev.so is missing: build() makes it"
    L.trgt_dev_consensus_vote.restype = C.c_int
    L.trgt_dev_consensus_vote.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 3
    ctx = _lib.Context(0, creator=L)
    yield ctx, L
    ctx.close()


def vote(dev_ctx, groups, out_cap=None, count_on_device=False):
    """groups: [(backbone, [(member, ops)])] in ONE launch of trgt_dev_consensus_vote -> [(raw length word, bytes)]"""
    ctx, L = dev_ctx
    blob, bb_off, bb_len, first, m_off, m_len, cig, cfirst, room = bytearray(), [], [], [0], [], [], [], [0], [0]
    for backbone, members in groups:
        bb_off.append(len(blob)); bb_len.append(len(backbone)); blob += backbone.encode()
        for member, ops in members:
            m_off.append(len(blob)); m_len.append(len(member)); blob += member.encode()
            cig += cases.words(ops)
            cfirst.append(len(cig))
        first.append(len(m_off))
        room.append(room[-1] + len(backbone) + sum(len(m) for m, _ in members) + 16)
    a = lambda v, t: np.array(v, t)
    blob_a = np.frombuffer(bytes(blob), np.uint8).copy()
    arrs = [a(bb_off, np.uint64), a(bb_len, np.uint32), a(first, np.uint64), a(m_off, np.uint64), a(m_len, np.uint32), a(cig + [0], np.uint32),
            a(cfirst, np.uint64)]
    caps = None if out_cap is None else a(out_cap, np.uint32)
    out_len, out_bytes, out_off = np.zeros(len(groups), np.uint32), np.zeros(room[-1], np.uint8), a(room, np.uint64)
    rc = L.trgt_dev_consensus_vote(ctx.handle, len(groups), blob_a.ctypes.data, len(blob_a), *[x.ctypes.data for x in arrs],
                                   None if caps is None else caps.ctypes.data, int(count_on_device), out_len.ctypes.data, out_bytes.ctypes.data,
                                   out_off.ctypes.data)
    assert rc == 0, (rc, L.trgt_hip_last_error(ctx.handle))
    return [(int(out_len[g]), bytes(out_bytes[room[g]:room[g] + int(out_len[g])]).decode() if out_len[g] != NO_FIT else None)
            for g in range(len(groups))]


_LISTS = {}


def group_list(name):
    """(groups, restated consensus of each), computed once"""
    if name not in _LISTS:
        if name == "hand":
            groups, want = [(b, m) for _, b, m, _ in cases.HAND], [e for _, _, _, e in cases.HAND]
        elif name == "shapes":
            groups, want = [(b, m) for _, b, m, _ in cases.SHAPES], [e for _, _, _, e in cases.SHAPES]
        else:
            groups = cases.random_groups(int(name.split("-")[1]))
            want = None
        restated = [restate(b, m) for b, m in groups]
        assert want is None or restated == want
        _LISTS[name] = (groups, restated)
    return _LISTS[name]


@pytest.mark.parametrize("count_on_device", [False, True], ids=["count on the host", "count on the device"])
@pytest.mark.parametrize("name", ["hand", "shapes"] + ["random-%d" % s for s in cases.RANDOM_SEEDS])
def test_lists_through_the_dev_entry(dev_ctx, name, count_on_device):
    groups, want = group_list(name)
    got = vote(dev_ctx, groups, count_on_device=count_on_device)
    assert len(got) == len(groups)
    for g, ((n, seq), w) in enumerate(zip(got, want)):
        assert n == len(w) and seq == w, (name, g, n, seq, w)


def test_does_not_fit(dev_ctx):
    # three groups whose output slots adjoin: the middle one gets one byte less than its consensus needs
    shapes = {s[0]: s for s in cases.SHAPES}
    groups = [(shapes[k][1], shapes[k][2]) for k in ("ends of 257", "candidates at the wave ballots' ends", "runs of 65 = and 130 D")]
    want = [restate(b, m) for b, m in groups]
    got = vote(dev_ctx, groups, out_cap=[0, len(want[1]) - 1, 0])
    assert got[1] == (NO_FIT, None)
    assert got[0] == (len(want[0]), want[0]) and got[2] == (len(want[2]), want[2])
    got = vote(dev_ctx, groups, out_cap=[0, len(want[1]), 0])  # ... and with exactly that much room it fits
    assert [s for _, s in got] == want


def test_repeatable_at_2048_members(dev_ctx):
    name, backbone, members, expected = cases.SHAPES[[s[0] for s in cases.SHAPES].index("2048 members")]
    first = vote(dev_ctx, [(backbone, members)])
    assert first == [(len(expected), expected)]
    assert vote(dev_ctx, [(backbone, members)]) == first


# ---------------------------------------------------------------------------------------------------------------- the release library
MAX_OPS = 10000  # genotype_cluster.rs:236


def _expected_allele(trs):
    """pyconsensus.make_consensus over all of trs: edit distances from WFAligner (score-only BiWFA, edit) with the MAX_OPS rule applied here,
    CIGARs from WFAligner (BiWFA, gap-affine 2,5,1) with the backbone as pattern"""
    from trgt_amd.wfaligner import AlignmentScope, MemoryModel, WFAligner
    n = len(trs)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    todo = [(i, j) for i, j in pairs if len(trs[i]) * len(trs[j]) <= MAX_OPS]
    score = {}
    if todo:
        ed = WFAligner.builder(AlignmentScope.Score, MemoryModel.MemoryUltraLow).edit().build()
        r = ed.align_end_to_end_batch([trs[i].encode() for i, _ in todo], [trs[j].encode() for _, j in todo], want_ops=False)
        assert (r["status"] == 0).all()
        score = {ij: abs(int(s)) for ij, s in zip(todo, r["score"])}
    dists = [float(np.sqrt(float(score[ij] if ij in score else abs(len(trs[ij[0]]) - len(trs[ij[1]]))))) for ij in pairs]

    def align(backbone, seqs):
        al = WFAligner.builder(AlignmentScope.Alignment, MemoryModel.MemoryUltraLow).affine(2, 5, 1).build()
        r = al.align_end_to_end_batch([backbone.encode()] * len(seqs), [s.encode() for s in seqs], want_ops=False)
        assert (r["status"] == 0).all()
        return [WFAligner.decode_sam_cigar(r["cigar"][int(r["cigar_off"][k]):int(r["cigar_off"][k]) + int(r["cigar_len"][k])]) for k in range(len(seqs))]
    return pyconsensus.make_consensus(n, trs, dists, list(range(n)), align), len(todo)


def test_release_library_designed_loci():
    from trgt_amd import locus
    _lib = _lib_mod()
    loci = cases.designed_loci()
    shallow = [L for L in loci if L["depth"] <= 256]
    assert sorted(L["depth"] for L in loci) == [1, 2, 3, 12, 30, 30, 300] and sum(L["long"] for L in loci) == 1
    params = locus.Params(max_depth=10000)
    expected = {}  # (locus, kept reads in the result's order) -> allele

    def check(ctx, which, n_device):
        b = locus.pack(which)
        out = locus.run_batch(b, params, ctx=ctx)
        n_ed = 0
        for l, L in enumerate(which):
            got = locus.locus_result(b, out, l)
            assert sorted(got.reads) == list(range(L["depth"])), l  # every read spans: every segment votes
            for r, (s, e) in zip(got.reads, got.tr_spans):
                assert L["reads"][r][s:e].decode() == L["segments"][r], (l, r)
            key = (loci.index(L), tuple(got.reads))
            if key not in expected:
                expected[key] = _expected_allele([L["segments"][r] for r in got.reads])
            want, n_pairs = expected[key]
            assert n_pairs == 0 if L["long"] else (n_pairs > 0 or L["depth"] == 1), (l, n_pairs)  # (MAX_OPS decides pair by pair)
            n_ed += n_pairs
            assert [a.seq.decode() for a in got.genotype] == [want], (l, L["depth"])
        # consensus alignments and edit distances ran on the GPU; loci the device chains genotyped
        print("consensus jobs %d, edit-distance jobs %d (%d reads, %d aligned pairs)" % (out.stats[1], out.stats[15], sum(L["depth"] for L in which), n_ed))
        assert int(out.stats[1]) > 0 and int(out.stats[15]) > 0, out.stats[:24]
        assert int(out.stats[22]) == n_device and int(out.stats[23]) == 0, out.stats[22:24]

    check(_lib.context(), shallow, len(shallow))  # the one-wave cluster chain
    host = _lib.context_with_env(TRGT_HOST_CLUSTER=1)  # consensus_repair_batch
    try:
        check(host, loci, 0)
    finally:
        host.close()
    deep = _lib.Context(0)  # the deep chain for the 300-read locus: the launch whose count is read from device memory
    try:
        deep.set_cluster_max_reads(_lib.cluster_max_reads_limit())
        check(deep, loci, len(loci))
    finally:
        deep.close()
