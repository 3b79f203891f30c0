"""The banded alignments of what the pre-filter keeps on one wave each, forward only (trgt_amd/csrc/wfa_band.hip: wfa_band_kernel), against
the three launches it replaces (heavy_band_kernel, wfa_fast_kernel<64, 3>, band_check_kernel: forced by TRGT_BAND_LDS=1 in the developer
library) and against the CPU oracle.

Everything goes through trgt_find_spans_batch with the hit bytes asked for (the sibling rules are then off: every missed piece gets its
alignment).  A read that ends inside a piece has no seeded window on the expensive list (the window would leave the read), so its job meets
the pre-filter, which hands penalty and end diagonal to the banded launch.  Every locus holds two long reads with both flanks, which make
the others "too short to span the locus"; every cut read holds its other piece exactly, so that the span of the cut piece's alignment shows
as the read's span.  The `[spans+]` lines say where the jobs went."""
import re

import numpy as np
import pytest

from helpers import rand_dna
from test_window_reg_gpu import _flank, _oracle_spans, _sub

pytestmark = pytest.mark.gpu

F = 250
TR = b"CAG" * 20
NAMES = ("span_start", "span_end", "lf_hit", "rf_hit")


def _locus(rng, lf, rf, reads, pad=330):
    anchors = [rand_dna(rng, pad) + lf + TR + rf + rand_dna(rng, pad), rand_dna(rng, pad - 10) + lf + TR + rf + rand_dna(rng, pad - 5)]
    longest = max(len(a) for a in anchors)
    assert all(len(r) < longest - (len(lf) + len(lf) // 5) for r in reads), (longest, sorted(len(r) for r in reads))
    return dict(left_flank=lf, right_flank=rf, tr=TR, motifs=[b"CAG"], ploidy=2, reads=list(reads) + anchors)


def _cut_right(rng, lf, piece, ov, head=150):
    """the read ends `ov` bases into `piece` (the right piece, possibly damaged)"""
    return rand_dna(rng, head) + lf + TR + piece[:ov]


def _cut_left(rng, piece, rf, ov, tail=150):
    """the read opens with the last `ov` bases of `piece` (the left piece, possibly damaged)"""
    return piece[len(piece) - ov:] + TR + rf + rand_dna(rng, tail)


def _lines(err):
    out = dict(kept=None, launch=None, long=None)
    for l in err.splitlines():
        if l.startswith("[spans+] kept by the pre-filter"):
            out["kept"] = tuple(int(t) for t in re.findall(r"\d+", l.split(":", 1)[1]))  # kept, banded, did not stand, whole read
        if l.startswith("[spans+] banded launch:"):
            out["launch"] = ("forward" if "forward only" in l else "lds",) + tuple(int(t) for t in re.findall(r"\d+", l.split(",", 1)[1]))
        if l.startswith("[spans+] long reads kept by the window filter"):
            out["long"] = tuple(int(t) for t in re.findall(r"\d+", l.split(":", 1)[1]))
    return out


def _run(loci, frac, flank_len, env):
    from trgt_amd import _lib, locus
    b = locus.pack(loci)
    p = locus.Params(min_flank_id_frac=frac, search_flank_len=flank_len)
    ctx = _lib.context_with_env(TRGT_WFA_DEBUG=1, **env)
    try:
        return locus.find_tr_spans_batch(b, p, ctx=ctx)
    finally:
        ctx.close()


def _three_ways(oracle, capfd, loci, frac=0.7, flank_len=F, env=None, with_oracle=True):
    """new launch, old launches, oracle: equal array for array.  Returns (lines of the new call, lines of the old call, new result)."""
    env = dict(env or {})
    capfd.readouterr()
    got_new = _run(loci, frac, flank_len, env)
    new = _lines(capfd.readouterr().err)
    got_old = _run(loci, frac, flank_len, dict(env, TRGT_BAND_LDS=1))
    old = _lines(capfd.readouterr().err)
    print("new", new, "old", old)
    for name, g, o in zip(NAMES, got_new, got_old):
        assert np.array_equal(g, o), (name, np.nonzero(g != o)[0][:10], g[g != o][:10], o[g != o][:10])
    if with_oracle:
        ref = _oracle_spans(oracle, loci, frac, flank_len)
        for name, g, r in zip(NAMES, got_new, ref):
            assert np.array_equal(g, r), (name, np.nonzero(g != r)[0][:10], g[g != r][:10], r[g != r][:10])
    assert new["kept"] == old["kept"], (new, old)
    if new["launch"] is not None:
        assert new["launch"][0] == "forward" and old["launch"][0] == "lds", (new, old)
    return new, old, got_new


def _pairs(rng, damage, overlaps, **kw):
    """per overlap one locus with a right-cut and a left-cut read; damage(piece, ov, side) returns the piece as the read holds it"""
    loci = []
    for ov in overlaps:
        lf, rf = _flank(rng), _flank(rng)
        loci.append(_locus(rng, lf, rf, [_cut_right(rng, lf, damage(rf, ov, "right"), ov), _cut_left(rng, damage(lf, ov, "left"), rf, ov)], **kw))
    return loci


def test_plain_cut_reads(oracle, capfd):
    """Exact overlaps of 174 .. 249 bases: penalty 5 + (250 - overlap), 175 matches are the threshold."""
    rng = np.random.default_rng(20261020)
    ovs = (174, 175, 176, 200, 249)
    loci = _pairs(rng, lambda p, ov, side: p, ovs)
    new, old, got = _three_ways(oracle, capfd, loci)
    kept, banded, failed, whole = new["kept"]
    # (the eight pieces with 175 matches or more must be kept and banded.  The two with 174 are below the threshold: the pre-filter, which
    #  this launch does not touch, drops them for this seed -- its bound on count_matches() is tight here -- for both launches alike)
    assert (kept, banded, failed, whole) == (8, 8, 0, 0), new
    assert new["launch"] == ("forward", 0, 0)
    ss = got[0].reshape(len(ovs), 4)
    assert (ss[0, :2] == -1).all() and (ss[1:, :2] >= 0).all() and (ss[:, 2:] >= 0).all()  # 174 matches: no span; all others span


def _at_cut(piece, ov, side, offsets, rng):
    """substitutions `offsets` bases away from the cut, inside the overlap (0: the last overlapped base)"""
    pos = [ov - 1 - o for o in offsets] if side == "right" else [len(piece) - ov + o for o in offsets]
    return _sub(rng, piece, pos)


@pytest.mark.parametrize("offsets", [(0,), (1,), (2,), (0, 3), (1, 4), (2, 4)])
def test_ties_at_the_cut(oracle, capfd, offsets):
    """A mismatch near the cut against more deleted bases: with x = 2 and e = 1 the second-to-last base is a tie, the third-to-last is not."""
    rng = np.random.default_rng(100 + sum(offsets))
    loci = _pairs(rng, lambda p, ov, side: _at_cut(p, ov, side, offsets, rng), (190, 221))
    for frac in (0.7, 188.5 / F, 189.5 / F, 186.5 / F, 187.5 / F):  # (count_matches() of the co-optimal alignments differs: thresholds around 187 .. 189)
        new, old, got = _three_ways(oracle, capfd, loci, frac=frac)
        kept, banded, failed, whole = new["kept"]
        assert failed == 0 and whole == 0 and banded == kept and new["launch"] == ("forward", 0, 0), new
        # at 0.7 all four cut pieces (188 matches at least) pass the threshold and must be kept and banded; the thresholds around the
        # shorter overlap decide about its two pieces, the two with an overlap of 221 bases always pass
        assert banded == 4 if frac == 0.7 else 2 <= banded <= 4, (frac, new)


def test_repeats_and_second_gaps_at_the_cut(oracle, capfd):
    """A homopolymer and a dinucleotide repeat across the cut point (the gap's place is open); a one-base insertion and a one-base deletion
    inside the overlap next to the cut's gap."""
    rng = np.random.default_rng(77)
    loci = []
    for unit, n in ((b"A", 14), (b"AC", 16), (b"GT", 9)):
        for ov in (200, 207):
            lf, rf = bytearray(_flank(rng)), bytearray(_flank(rng))
            rf[ov - n // 2:ov - n // 2 + n] = (unit * n)[:n]
            lf[F - ov - n // 2:F - ov - n // 2 + n] = (unit * n)[:n]
            lf, rf = bytes(lf), bytes(rf)
            loci.append(_locus(rng, lf, rf, [_cut_right(rng, lf, rf, ov), _cut_left(rng, lf, rf, ov)]))
    for at in (30, 120, 195):
        lf, rf = _flank(rng), _flank(rng)
        ins_r, del_r = rf[:at] + b"T" + rf[at:], rf[:at] + rf[at + 1:]
        ins_l, del_l = lf[:F - at] + b"G" + lf[F - at:], lf[:F - at - 1] + lf[F - at:]
        loci.append(_locus(rng, lf, rf, [_cut_right(rng, lf, ins_r, 211), _cut_right(rng, lf, del_r, 209),
                                         _cut_left(rng, ins_l, rf, 211), _cut_left(rng, del_l, rf, 209)]))
    new, old, got = _three_ways(oracle, capfd, loci)
    kept, banded, failed, whole = new["kept"]
    assert failed == 0 and whole == 0 and banded == kept == 12 + 12, new
    assert (got[0] >= 0).all()


CAP = 96


@pytest.mark.parametrize("band", [None, "20", "256"])
def test_cap_edges(oracle, capfd, band):
    """Penalties CAP - 1, CAP and CAP + 1 (overlaps of 160, 159, 158 bases; threshold 150) and two below 20.  By default the plan's bound is
    the kernel's cap: CAP + 1 goes whole-read.  With TRGT_HEAVY_BAND=256 it is banded by the LDS launch behind the kernel; with 20
    everything above 20 goes whole-read."""
    rng = np.random.default_rng(5)
    ovs = (F + 5 - (CAP - 1), F + 5 - CAP, F + 5 - (CAP + 1), 240, 236)
    loci = _pairs(rng, lambda p, ov, side: p, ovs)
    new, old, got = _three_ways(oracle, capfd, loci, frac=0.6, env={} if band is None else dict(TRGT_HEAVY_BAND=band))
    kept, banded, failed, whole = new["kept"]
    assert failed == 0 and kept == 10, new
    if band is None:
        assert (banded, whole) == (8, 2) and new["launch"] == ("forward", 0, 0), new
    elif band == "20":
        assert (banded, whole) == (4, 6) and new["launch"] == ("forward", 0, 0), new
    else:
        assert (banded, whole) == (10, 0) and new["launch"] == ("forward", 2, 0), new
    assert (got[0] >= 0).all()


def _clipped_k_hi_loci(rng):
    """Reads that hold nothing of a 40-base right piece but its first c = 2 .. 5 bases, as their last bases: the piece is written in A and C,
    the rest of the read in G and T (and the left piece in N and R), so no other base of it can match.  The alignment is those c matches and a deletion of the other
    40 - c bases: penalty 45 - c >= 40, the pattern consumed where the read ends, on the diagonal k_end = rlen - 40.  Then
    k_end + s* >= rlen: the start diagonals are clipped by the end of the read (k_hi = rlen) as the window is (t_end = rlen), the free text
    start is the whole window (tbf = tlen) and the last start diagonal has h = tlen at v = 0."""
    loci, cut_reads = [], []
    for c in (2, 3, 4, 5, 5, 3):
        lf = bytes(rng.choice(list(b"NR"), 40).astype(np.uint8))  # (the left piece shares no byte with these reads: no job of it is kept)
        rf = bytes(rng.choice(list(b"AC"), 40).astype(np.uint8))
        read = bytes(rng.choice(list(b"GT"), int(rng.integers(100, 140))).astype(np.uint8)) + rf[:c]
        loci.append(_locus(rng, lf, rf, [read], pad=120))
        cut_reads.append((rf, read, c))
    return loci, cut_reads


def test_band_clipped_by_the_end_of_the_read_at_k_hi(oracle, capfd):
    """t_end = tlen AND k_hi = tlen: see _clipped_k_hi_loci.  The oracle says that every case is what it claims.  Threshold 2 of 40 matches,
    so every right piece is an aligned hit; the left piece is nowhere in the read, so no read spans and the hit bytes carry the result."""
    rng = np.random.default_rng(4040)
    loci, cut_reads = _clipped_k_hi_loci(rng)
    for rf, read, c in cut_reads:
        p = oracle.wfa_params("affine", x=2, o1=5, e1=1, span="endsfree", pbf=0, pef=0, tbf=len(read), tef=len(read), heuristic="none")
        a = oracle.wfa_align(p, rf, read)
        s, k_end = abs(a["score"]), len(read) - 40
        assert s == 45 - c and a["n_match"] == c and a["span"] == [0, c, len(read) - c, len(read)], (c, a["score"], a["span"], a["n_match"])
        assert 40 <= s <= CAP and k_end - s > 0 and k_end + s >= len(read)  # clipped at the end only: t0 > 0, k_hi = t_end = rlen
    new, old, got = _three_ways(oracle, capfd, loci, frac=0.05, flank_len=40)
    kept, banded, failed, whole = new["kept"]
    assert (kept, banded, failed, whole) == (len(loci), len(loci), 0, 0), new
    assert new["launch"] == ("forward", 0, 0), new
    assert (got[3].reshape(len(loci), 3)[:, 0] == 2).all() and (got[2].reshape(len(loci), 3)[:, 0] == 0).all()


def test_short_flanks_and_clipped_bands(oracle, capfd):
    """Flank length 40 (no seed search at all: every job of a short read meets the pre-filter).  Left cuts have their band clipped by the
    start of the read (t0 = 0), right cuts by its end (t_end = tlen; k_hi clipped as well: test_band_clipped_by_the_end_of_the_read_at_k_hi)."""
    rng = np.random.default_rng(40)
    loci = []
    for ov in (22, 25, 31, 39):
        lf, rf = rand_dna(rng, 40), rand_dna(rng, 40)
        loci.append(_locus(rng, lf, rf, [_cut_right(rng, lf, rf, ov, head=int(rng.integers(5, 60))), _cut_left(rng, lf, rf, ov, tail=int(rng.integers(5, 60))),
                                         rand_dna(rng, 30) + _sub(rng, lf, [7, 20, 33]) + TR + _sub(rng, rf, [3, 30]) + rand_dna(rng, 25)], pad=120))
    new, old, got = _three_ways(oracle, capfd, loci, frac=0.5, flank_len=40)
    kept, banded, failed, whole = new["kept"]
    # per locus: the two cut pieces and both pieces of the third read (their substitutions leave no exact match; no seed search at 40)
    assert (kept, banded, failed, whole) == (16, 16, 0, 0) and new["launch"] == ("forward", 0, 0), new
    assert (got[0] >= 0).all()


def test_long_flanks_take_the_lds_launch(oracle, capfd):
    """Pieces beyond 255 bases.  The pre-filter takes pieces of up to 254 bases (flank_filter_max_tlen), so span_plan() plans neither it nor
    the band for such a call: no flank length reaches the kernel's own hand-over of long pieces.  Should a later pre-filter take them,
    every banded job must go through the LDS launch; until then the call must not name a band at all, and the results are the oracle's."""
    rng = np.random.default_rng(300)
    n = 300
    loci = []
    for ov in (260, 290):
        lf, rf = rand_dna(rng, n), rand_dna(rng, n)
        loci.append(_locus(rng, lf, rf, [_cut_right(rng, lf, rf, ov), _cut_left(rng, lf, rf, ov)], pad=400))
    new, old, got = _three_ways(oracle, capfd, loci, flank_len=n)
    if new["kept"] is not None:  # (a plan that bands these pieces)
        kept, banded, failed, whole = new["kept"]
        assert failed == 0 and new["launch"] == ("forward", banded, 0), new
    else:
        assert new["launch"] is None and old["launch"] is None
    assert (got[0] >= 0).all()


def test_other_bytes(oracle, capfd):
    """N, lower case and a zero byte in piece and read."""
    rng = np.random.default_rng(9)
    loci = []
    for ov in (205, 230):
        lf, rf = bytearray(_flank(rng)), bytearray(_flank(rng))
        for q in (rf, lf):
            q[60] = ord("N"); q[61] = ord("N"); q[150] = ord("a"); q[199] = 0
        lf, rf = bytes(lf), bytes(rf)
        dr, dl = bytearray(rf), bytearray(lf)
        dr[100] = ord("N"); dl[180] = ord("n")
        loci.append(_locus(rng, lf, rf, [_cut_right(rng, lf, bytes(dr), ov), _cut_left(rng, bytes(dl), rf, ov)]))
    new, old, got = _three_ways(oracle, capfd, loci)
    kept, banded, failed, whole = new["kept"]
    assert failed == 0 and whole == 0 and banded == kept == 4, new
    assert (got[0] >= 0).all()


def test_long_reads(oracle, capfd):
    """Four loci with reads of kilobases whose windows name penalty and end diagonal: the long reads' band."""
    rng = np.random.default_rng(3000)
    loci = []
    for li in range(4):
        lf, rf = _flank(rng), _flank(rng)
        tr = (b"CAG" * 1200)[:int(rng.integers(2900, 3300))]
        reads = [rand_dna(rng, 300) + _sub(rng, lf, [int(v) for v in rng.choice(F, 12 + 6 * i, replace=False)]) + tr + _sub(rng, rf, [11, 99, 201]) + rand_dna(rng, 200) for i in range(4)]
        reads.append(lf[60:] + tr + rf + rand_dna(rng, 100))
        reads.append(rand_dna(rng, 100) + lf + tr + rf[:200])
        loci.append(dict(left_flank=lf, right_flank=rf, tr=TR, motifs=[b"CAG"], ploidy=2, reads=reads))
    new, old, got = _three_ways(oracle, capfd, loci)
    # per locus the four damaged left pieces (12 .. 30 substitutions: penalty above the seeded windows' 15) and the two cut pieces
    assert new["long"] == old["long"] == (24, 0), (new, old)
    assert new["launch"] == ("forward", 0, 0) and old["launch"] == ("lds", 0, 0), (new, old)
    assert new["kept"] is None or new["kept"][2] == 0, new


def test_random_cut_reads_against_the_lds_launch(oracle, capfd):
    """2 000 cut reads: cut point uniform over the piece, substitutions / insertions / deletions at 0 - 3 % each."""
    rng = np.random.default_rng(20261021)

    def noisy(seq):
        out = bytearray()
        rs, ri, rd = (float(rng.uniform(0, 0.03)) for _ in range(3))
        for c in seq:
            u = rng.random()
            if u < rd:
                continue
            if u < rd + ri:
                out += rand_dna(rng, 1)
            out.append(int(rng.choice([x for x in b"ACGT" if x != c])) if rng.random() < rs else c)
        return bytes(out)

    loci = []
    for _ in range(100):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        reads = []
        for i in range(20):
            cut = int(rng.integers(1, F))
            if i & 1:
                reads.append(rand_dna(rng, int(rng.integers(0, 200))) + noisy(lf) + TR + noisy(rf[:cut]))
            else:
                reads.append(noisy(lf[cut:]) + TR + noisy(rf) + rand_dna(rng, int(rng.integers(0, 200))))
        loci.append(_locus(rng, lf, rf, reads))
    new, old, got = _three_ways(oracle, capfd, loci, with_oracle=False)
    kept, banded, failed, whole = new["kept"]
    assert failed == 0 and banded >= 400 and kept == banded + whole, new
