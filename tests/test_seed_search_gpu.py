"""The seed search of the flank location (trgt_amd/csrc/spans.hip: piece_window_heads in flank_window_kernel): which (position,
segment) pairs count as seeds, and with them kmin / kmax.  A search that misses a seed, or takes one that is none, costs time only --
the whole-read launch still gives the right answer -- so every batch is checked twice: the results array for array against the oracle
(the locus path, host reads and reads in HBM), and the ROUTING of the fallback alignments, the counts of the TRGT_WFA_DEBUG line
`[spans]` (windowed, whole read, settled by the shortcuts, of those one-base gaps), against a prediction for the constructed batch.

The prediction restates the routing on the host: the exact scan and its sibling rule decide which pieces are jobs and on which list
(reads at least heavy_read_len of their locus: the light one); tools/sibling_census.py (seed_plan, seeded_diagonals, front_search) gives
the seeds and the shortcuts; the light list windows a job when kmax - kmin <= spread, the front list only with the piece inside the
read; a window stands when the optimal penalty over the whole read is within the bound S0 = 2 segments - 1 (the oracle's aligner says
which).  The counts must be equal to the job."""
import os
import sys

import numpy as np
import pytest

from helpers import rand_dna

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sibling_census as census  # noqa: E402

pytestmark = pytest.mark.gpu

F = 250
SCORING = (2, 5, 1)
MIN_MATCHES = 175     # ceil(0.7 F): the scan's sibling rule
ANCHOR = 1220         # two plain reads of this length per locus: the reads under test from 920 bases on are on the light list


def _sub(rng, seq, positions):
    b = bytearray(seq)
    for p in positions:
        b[p] = int(rng.choice([c for c in b"ACGT" if c != b[p]]))
    return bytes(b)


def _other(rng, seq):
    """as long as seq, every base another one"""
    return _sub(rng, seq, range(len(seq)))


def _spoil_heads(rng, flank, segments, q, at=3):
    """a substitution inside the first twelve bases of each of the given segments: none of them seeds"""
    return _sub(rng, flank, [s * q + at for s in segments])


def _locus(rng, lf, rf, reads, anchors=True, anchors_first=False):
    tr = b"CAG" * 20
    extra = []
    if anchors:
        extra = [rand_dna(rng, (ANCHOR - 560) // 2) + lf + tr + rf + rand_dna(rng, ANCHOR - 560 - (ANCHOR - 560) // 2) for _ in range(2)]
    reads = extra + list(reads) if anchors_first else list(reads) + extra
    assert len(reads) <= 16 and max(len(r) for r in reads) <= 1230  # (longer reads are on a list of their own, which is not modelled here)
    return dict(left_flank=lf, right_flank=rf, tr=tr, motifs=[b"CAG"], ploidy=2, reads=reads)


def _penalty(oracle, piece, read):
    x, o, e = SCORING
    p = oracle.wfa_params("affine", x=x, o1=o, e1=e, span="endsfree", pbf=0, pef=0, tbf=len(read), tef=len(read), heuristic="none")
    return abs(oracle.wfa_align(p, piece, read)["score"])


def _predict(oracle, loci, segments=8):
    """(windowed, whole read, settled by the shortcuts, of those one-base gaps) of the `[spans]` line for these loci"""
    plan = census.seed_plan(F, *SCORING, segments=segments)
    assert plan["ok"] and plan["hamming_max"] == 2 and plan["indel_ok"]
    s0 = SCORING[0] * segments - 1
    windowed = whole = settled = gaps = 0
    for L in loci:
        pieces = (L["left_flank"][-F:], L["right_flank"][:F])
        longest = max(len(r) for r in L["reads"])
        heavy_len = max(longest - (F + F // 5), 0)
        for read in L["reads"]:
            n = len(read)
            pos = [read.find(pieces[0]), read.find(pieces[1])]
            for side in (0, 1):
                if pos[side] >= 0:
                    continue
                sib = pos[side ^ 1]
                if sib >= 0 and (n - sib - F if side else sib) < MIN_MATCHES:
                    continue  # the sibling rule: no job
                front = n < heavy_len
                kind = census.front_search(read, pieces[side], plan)
                if kind[0] == "noseed" and not front:
                    kk = census.seeded_diagonals(read, pieces[side], plan)
                    if kk is not None and kk[1] - kk[0] <= plan["spread"]:
                        kind = ("window",)
                if kind[0] == "settled":
                    settled += 1
                    gaps += kind[2] - kind[1] != F
                elif kind[0] == "window":
                    windowed += 1
                    whole += _penalty(oracle, pieces[side], read) > s0  # a window that does not stand
                elif not front:
                    whole += 1
    return windowed, whole, settled, gaps


def _spans_counts(err):
    out = []
    for line in err.splitlines():
        if line.startswith("[spans] fallback alignments"):
            nums = [int(t) for t in line.replace(",", " ").replace("(", " ").replace(")", " ").split() if t.isdigit()]
            # first launch, long reads, light, windowed, whole read, without seeds, did not stand, settled, one-base gaps
            assert len(nums) == 9, line
            out.append(((nums[3], nums[4], nums[7], nums[8]), line))
    return out


def _check(oracle, capfd, loci, segments=8):
    """results against the oracle (host reads, reads in HBM) and the routing of both runs against the prediction"""
    import torch
    from trgt_amd import _lib, locus
    from test_locus_gpu import _compare
    want = _predict(oracle, loci, segments)
    b = locus.pack(loci)
    p = locus.Params()
    env = dict(TRGT_WFA_DEBUG=1)
    if segments != 8:
        env["TRGT_WIN_SEGMENTS"] = segments
    ctx = _lib.context_with_env(**env)
    try:
        capfd.readouterr()
        reads_dev = torch.from_numpy(b["read_blob"]).cuda()  # (allocated to the exact size of the blob)
        outs = [locus.run_batch(b, p, ctx=ctx),
                locus.run_batch(b, p, ctx=ctx, flank_dev=torch.from_numpy(b["flank_blob"]).cuda(), reads_dev=reads_dev)]
        for out in outs:
            _compare(oracle, locus, b, out, p, range(len(loci)))
    finally:
        ctx.close()
    got = _spans_counts(capfd.readouterr().err)
    assert len(got) == 2, got
    for counts, line in got:
        print("predicted (windowed, whole read, settled, gaps) %s: %s" % (want, line))
        assert counts == want, (want, line)
    return want


@pytest.mark.parametrize("period", [1, 2, 4, 8, 16, 3, 5, 13])
def test_several_lanes_at_one_position(oracle, capfd, period):
    """Periodic flanks: with period 1, 2, 4, 8 and 16 several lanes match at the same one of a lane's sixteen positions, with period 3, 5
    and 13 a lane matches at several.  Each flank carries one substitution, every fourth read has one period deleted."""
    rng = np.random.default_rng(700 + period)
    loci = []
    for _ in range(2):
        unit = rand_dna(rng, period)
        while period > 1 and len(set(unit)) == 1:
            unit = rand_dna(rng, period)
        lf, rf = (unit * (F // period + 1))[:F], rand_dna(rng, F)
        reads = []
        for i in range(8):
            l = _sub(rng, lf, [9 + 29 * i])
            if i % 4 == 3:
                l = l[:60] + l[60 + period:]
            r = _sub(rng, rf, [50 + i])
            if i % 4 == 1:
                r = r[:130] + r[131:]
            reads.append(rand_dna(rng, 290 + i) + l + b"CAG" * 20 + r + rand_dna(rng, 310))
        loci.append(_locus(rng, lf, rf, reads))
    _check(oracle, capfd, loci)


def test_spread_at_the_bound(oracle, capfd):
    """kmin and kmax themselves: the left flank seeds with its last segment only, on diagonal A (its window would stand: penalty 14), and
    the head of the first segment is planted in front of it on the diagonals A - d.  With every d <= 20 = spread the read is windowed,
    with one of 21 and more it is not; d = 16 and 32 put several lanes on one of a lane's sixteen positions, the other pairs two
    positions into neighbouring lanes."""
    rng = np.random.default_rng(2021)
    q, loci = F // 8, []
    plants = ([16], [20], [21], [16, 32], [12, 24], [13, 29], [17, 33], [24], [12], [19], [15, 31], [20, 36])  # (twelve bases each: no overlap)
    for k in range(2):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        reads = []
        for j, ds in enumerate(plants):
            A = 400 + 16 * k + 7 * j
            head = bytearray(rand_dna(rng, A))
            for d in ds:
                head[A - d:A - d + 12] = lf[:12]
            reads.append(bytes(head) + _spoil_heads(rng, lf, range(7), q, at=2 + j % 9) + rand_dna(rng, 330))
        loci.append(_locus(rng, lf, rf, reads))
    want = _check(oracle, capfd, loci)
    assert want[0] == 2 * sum(max(ds) <= 20 for ds in plants)


def _collision_reads(rng, lf, rf, q, segments, n_reads):
    """the left flank without a seed of its own; in front of it, at 24 places, the first four bytes of a segment head followed by other
    bytes 5-8, or the first eight followed by other bytes 9-12 -- and in every second read one place where all twelve match"""
    reads = []
    for i in range(n_reads):
        l = _spoil_heads(rng, lf, range(segments), q, at=1 + i % 11)
        head = bytearray(rand_dna(rng, 420))
        for j in range(24):
            s = (i + j) % segments
            h = lf[s * q:s * q + 12]
            decoy = h[:4] + _other(rng, h[4:8]) + h[8:] if j % 2 else h[:8] + _other(rng, h[8:])
            if j % 6 == 5:
                decoy = h[:4] + _other(rng, h[4:])
            at = 3 + 17 * j + (i + j) % 5  # (every residue of the position mod 16 and mod 4 over the batch)
            head[at:at + 12] = decoy
        if i % 2 == 0:
            s = i // 2 % segments
            at = 3 + 17 * 24 + i
            head[at - 8:at - 4] = lf[s * q:s * q + 4]  # (and the first dword once more, eight bytes in front of it)
            head[at:at + 12] = lf[s * q:s * q + 12]
        reads.append(bytes(head) + l + b"CAG" * 20 + _sub(rng, rf, [77]) + rand_dna(rng, 220))
    return reads


def test_head_collisions(oracle, capfd):
    rng = np.random.default_rng(4112)
    loci = []
    for _ in range(2):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        loci.append(_locus(rng, lf, rf, _collision_reads(rng, lf, rf, F // 8, 8, 12)))
    want = _check(oracle, capfd, loci)
    assert want[0] == 12 and want[2] == 24  # the six full heads per locus window their read; every right flank is settled


def _end_reads(rng, lf, n, q, segments):
    """reads of n bases, nothing of either flank in them but one head of a segment: whole with its start at last = n - 12 and at
    last - 1, and cut by the end of the read with its start at last + 1 .. n - 4"""
    reads = []
    for j, start in enumerate(range(n - 13, n - 3)):
        s = (j + n) % segments
        h = lf[s * q:s * q + 12]
        reads.append(rand_dna(rng, start) + h[:n - start])
    return reads


def test_the_end_of_the_read(oracle, capfd):
    """The last seed starts at last = n - 12; a head that starts behind it is cut by the end of the read and does not count.  Read
    lengths of every residue mod 4 and of 0, 11, 12 and 15 mod 16, so that the end falls at every place of the lane that crosses it."""
    rng = np.random.default_rng(1212)
    loci = []
    for n in (928, 939, 940, 943, 929, 930):  # mod 16: 0, 11, 12, 15, 1, 2
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        loci.append(_locus(rng, lf, rf, _end_reads(rng, lf, n, F // 8, 8)))
    want = _check(oracle, capfd, loci)
    assert want[0] == 2 * len(loci)  # the two whole heads per length


def test_reads_of_a_few_bases(oracle, capfd):
    """Reads of 12, 13, 27, 28 and 29 bases (one candidate start, two, and the three lengths around the 28 bytes a lane loads) hold a
    segment head at their start or flush with their end; below 12 bases no search runs.  Loci of such reads only: all on the light list."""
    rng = np.random.default_rng(29)
    loci = []
    for k in range(3):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        q, reads = F // 8, []
        for j, n in enumerate((12, 13, 27, 28, 29)):
            h = lf[(j + k) % 8 * q:][:12]
            reads += [h + rand_dna(rng, n - 12), rand_dna(rng, n - 12) + h]
        reads += [lf[:11], lf[q:q + 5], rf[:4], rand_dna(rng, 1)]
        loci.append(_locus(rng, lf, rf, reads, anchors=False))
    # (a batch of such reads alone has no seeded windows at all: one locus with reads of ordinary length)
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    loci.append(_locus(rng, lf, rf, [rand_dna(rng, 300) + _sub(rng, lf, [40]) + b"CAG" * 20 + rf + rand_dna(rng, 320)]))
    want = _check(oracle, capfd, loci)
    assert want[0] >= 27  # every read of 12 bases and more holds a head (the read of 12 that IS one is built twice)


def test_behind_the_end_of_the_read(oracle, capfd):
    """Read i ends with the first 4 to 11 bytes of a segment head; read i + 1, next in the blob, starts with the rest and then with a
    whole head.  Neither seeds read i.  The last read of the batch ends that way flush with the blob, and with the tensor that holds it."""
    rng = np.random.default_rng(411)
    loci, q = [], F // 8
    for k in range(2):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        reads = []
        for c in range(4 + 4 * k, 8 + 4 * k):
            s = (c + 3) % 8
            h = lf[s * q:s * q + 12]
            reads.append(rand_dna(rng, 925 + c) + h[:c])
            reads.append(h[c:] + h + rand_dna(rng, 930))
        loci.append(_locus(rng, lf, rf, reads, anchors_first=True))
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    loci.append(_locus(rng, lf, rf, [rand_dna(rng, 950) + lf[2 * q:2 * q + 11]], anchors_first=True))
    b_last = loci[-1]["reads"][-1]
    assert b_last.endswith(lf[2 * q:2 * q + 11])
    want = _check(oracle, capfd, loci)
    assert want[0] == 8  # the whole heads at the start of the reads i + 1, nothing else


def test_two_rounds(oracle, capfd):
    """Light reads of 1 040 to 1 230 bases whose only seed, the head of the last segment, starts at each of the positions 1 008 .. 1 024:
    the sixteen positions of lane 63, the last of which reach bytes beyond 1 024, and lane 0 of the second round."""
    rng = np.random.default_rng(1024)
    q, loci = F // 8, []
    positions = list(range(1008, 1025))
    for part in (positions[:9], positions[9:]):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        reads = []
        for j, p in enumerate(part):
            l = _spoil_heads(rng, lf, range(7), q, at=2 + j)  # penalty 14: its window stands
            reads.append(rand_dna(rng, p - 7 * q) + l + rand_dna(rng, 170 - 10 * j))
            assert reads[-1].find(lf[7 * q:7 * q + 12]) == p and 1030 <= len(reads[-1]) <= 1230
        loci.append(_locus(rng, lf, rf, reads))
    want = _check(oracle, capfd, loci)
    assert want[0] == 17 and want[1] == 17  # every left piece windowed and standing; every right piece, absent, over the whole read


def _overhang_reads(rng, lf, rf, total):
    """the piece starts before the read (k < 0) or ends behind it (k + F > n); reads of about `total` bases"""
    reads, tr = [], b"CAG" * 20
    for j, c in enumerate((1, 4, 7, 12, 40)):
        l = _sub(rng, lf, [100 + j])[c:]                 # penalty 2 + 5 + c
        reads.append(l + tr + rf + rand_dna(rng, total - 560 + c))
        r = _sub(rng, rf, [120 + j])[:F - c]
        reads.append(rand_dna(rng, total - 560 + c) + lf + tr + r)
    reads.append(lf[2:] + tr + rf[:F - 3] + rand_dna(rng, 0))  # both at once, no substitution; too short for either list's shortcuts
    return reads


def test_negative_and_overhanging_diagonals_light(oracle, capfd):
    rng = np.random.default_rng(77)
    loci = []
    for _ in range(2):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        reads = _overhang_reads(rng, lf, rf, 960)[:10]
        loci.append(_locus(rng, lf, rf, reads))
    want = _check(oracle, capfd, loci)
    assert want[0] == 20  # the light list windows them all; those that lack more than 8 bases do not stand


def test_negative_and_overhanging_diagonals_front(oracle, capfd):
    """... and on the front list (reads too short to span their locus), which windows a piece only inside the read"""
    rng = np.random.default_rng(78)
    loci = []
    for _ in range(2):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        reads = _overhang_reads(rng, lf, rf, 700)
        reads.append(rand_dna(rng, 60) + _sub(rng, lf, [30, 31, 200]) + b"CAG" * 20 + _sub(rng, rf, [9]) + rand_dna(rng, 55))  # inside: windowed, settled
        loci.append(_locus(rng, lf, rf, reads))
    want = _check(oracle, capfd, loci)
    assert want == (2, 0, 2, 0)


@pytest.mark.parametrize("segments", [4, 6])
def test_four_and_six_segments(oracle, capfd, segments):
    """flank_window_kernel<4> and <6> (TRGT_WIN_SEGMENTS): head collisions, the end of the read and the overhanging pieces once more"""
    rng = np.random.default_rng(segments)
    q, loci = F // segments, []
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    loci.append(_locus(rng, lf, rf, _collision_reads(rng, lf, rf, q, segments, 12)))
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    loci.append(_locus(rng, lf, rf, _end_reads(rng, lf, 939, q, segments)))
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    loci.append(_locus(rng, lf, rf, _overhang_reads(rng, lf, rf, 960)[:10]))
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    reads = []
    for i in range(12):  # substitutions and one-base gaps around the smaller bounds (7 and 11)
        l = _sub(rng, lf, [7 + 19 * j for j in range(i % 7)])
        r = rf[:40 + 13 * i] + rf[41 + 13 * i:] if i % 2 else rf[:90] + rf[89:]
        reads.append(rand_dna(rng, 300 + i) + l + b"CAG" * 20 + r + rand_dna(rng, 320))
    loci.append(_locus(rng, lf, rf, reads))
    _check(oracle, capfd, loci, segments)
