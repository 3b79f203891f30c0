"""The windowed flank alignments on one wave each, wavefronts and history in registers (trgt_amd/csrc/wfa_win.hip: wfa_win_kernel), against
the launch it replaces (wfa_fast_kernel<64, 2>, forced by TRGT_WIN_LDS=1 in the developer library) and against the CPU oracle.

Everything goes through the stand-alone entry trgt_find_spans_batch with the hit bytes asked for (the sibling rule is then off: every
missed piece gets its alignment).  The entry hands out, per read, the repeat span (end of the left piece, start of the right piece) and
the two hit bytes (0 none, 1 exact, 2 aligned) -- the per-piece exact position, count_matches() and alignment span stay inside the call
and show through these: every damaged flank is put once as the left and once as the right piece of a read whose other piece is exact, so
the end AND the start of its alignment span are compared, and count_matches() is pinned where co-optimal alignments differ in it by
moving the acceptance threshold to just below and just above the oracle's count.  The three results must be equal array for array.

Every hand-made read must really reach the windowed launch (no shortcut of the seed search takes it, the sibling rule is off): the
debug line's count of windowed alignments is compared with the number of constructed cases, the line of the windowed launch must name
the kernel that ran, and the register kernel must have handed on no alignment.

The kernel's own fall-back (a piece or window beyond its 496-byte staging buffers) is not reachable through the public parameters:
a window is at most flank_len + 70 bases, and the host takes the LDS launch for a whole call when flank_len + 70 > 496
(test_flank_beyond_the_staging_buffers_takes_the_lds_launch)."""
import numpy as np
import pytest

from helpers import rand_dna

pytestmark = pytest.mark.gpu

F = 250


def _sub(rng, seq, positions):
    b = bytearray(seq)
    for p in positions:
        b[p] = int(rng.choice([c for c in b"ACGT" if c != b[p]]))
    return bytes(b)


def _ins(rng, seq, at, n, what=None):
    return seq[:at] + (what if what is not None else rand_dna(rng, n)) + seq[at:]


def _del(seq, at, n):
    return seq[:at] + seq[at + n:]


def _flank(rng):
    """250 random bases without a homopolymer run of three (a gap then has one cheapest place unless the case builds a repeat itself)"""
    out = bytearray(rand_dna(rng, F))
    for i in range(2, F):
        while out[i] == out[i - 1] == out[i - 2]:
            out[i] = int(rng.choice(list(b"ACGT")))
    return bytes(out)


def _pair(flank, damaged, rng, head=None, tail=None, pre=b"", other=None):
    """One locus per side: `damaged` as the left piece of a read whose right piece is exact (its alignment's END shows as span start) and
    as the right piece of a read whose left piece is exact (its START shows as span end).  head / tail: the bases of the read in front
    of / behind the damaged piece on the side where it touches the end of the read (None: 150 random ones)."""
    other = other or _flank(rng)
    tr = b"CAG" * 20
    h = rand_dna(rng, 150) if head is None else head
    t = rand_dna(rng, 150) if tail is None else tail
    left = dict(left_flank=flank, right_flank=other, tr=tr, motifs=[b"CAG"], ploidy=2,
                reads=[h + pre + damaged + tr + other + rand_dna(rng, 100), rand_dna(rng, 100) + flank + tr + other + rand_dna(rng, 100)])
    right = dict(left_flank=other, right_flank=flank, tr=tr, motifs=[b"CAG"], ploidy=2,
                 reads=[rand_dna(rng, 130) + other + tr + pre + damaged + t, rand_dna(rng, 100) + other + tr + flank + rand_dna(rng, 100)])
    for L in (left, right):
        assert all(590 <= len(r) <= 900 for r in L["reads"]), [len(r) for r in L["reads"]]
    return [left, right]


def _penalty(oracle, flank, read):
    p = oracle.wfa_params("affine", x=2, o1=5, e1=1, span="endsfree", pbf=0, pef=0, tbf=len(read), tef=len(read), heuristic="none")
    return oracle.wfa_align(p, flank, read)


def _oracle_spans(oracle, loci, frac=0.7, flank_len=F):
    ss, se, lh, rh = [], [], [], []
    for L in loci:
        thr = float(flank_len) * frac
        ls, le, lu, _ = oracle.find_spans(L["left_flank"][-flank_len:], L["reads"], 2, 5, 1, threshold=thr)
        rs, re_, ru, _ = oracle.find_spans(L["right_flank"][:flank_len], L["reads"], 2, 5, 1, threshold=thr)
        for i in range(len(L["reads"])):
            hl = 0 if ls[i] < 0 else (2 if lu[i] else 1)
            hr = 0 if rs[i] < 0 else (2 if ru[i] else 1)
            both = hl and hr and le[i] <= rs[i]
            ss.append(int(le[i]) if both else -1); se.append(int(rs[i]) if both else -1)
            lh.append(hl); rh.append(hr)
    return np.array(ss, np.int32), np.array(se, np.int32), np.array(lh, np.uint8), np.array(rh, np.uint8)


def _debug_counts(err):
    """(windowed alignments, redone against the whole read, kernel of the windowed launch, alignments it did not take)"""
    line = [l for l in err.splitlines() if l.startswith("[spans]")][-1]
    nums = [int(t) for t in line.replace(",", " ").replace("(", " ").replace(")", " ").split() if t.isdigit()]
    wl = [l for l in err.splitlines() if l.startswith("[spans+] windowed launch:")][-1]
    return nums[3], nums[-3], ("registers" if "history in registers" in wl else "lds"), int(wl.split(",")[-1].split()[0])


def _three_ways(oracle, capfd, loci, frac=0.7, env=None, flank_len=F):
    """new launch, old launch, oracle: equal array for array.  Returns (windowed, redone) of the new launch's call."""
    from trgt_amd import _lib, locus
    b = locus.pack(loci)
    p = locus.Params(min_flank_id_frac=frac, search_flank_len=flank_len)
    env = dict(env or {})
    new = _lib.context_with_env(TRGT_WFA_DEBUG=1, **env)
    old = _lib.context_with_env(TRGT_WFA_DEBUG=1, TRGT_WIN_LDS=1, **env)
    try:
        capfd.readouterr()
        got_new = locus.find_tr_spans_batch(b, p, ctx=new)
        err_new = capfd.readouterr().err
        got_old = locus.find_tr_spans_batch(b, p, ctx=old)
        err_old = capfd.readouterr().err
    finally:
        new.close()
        old.close()
    ref = _oracle_spans(oracle, loci, frac, flank_len)
    for name, g, o in zip(("span_start", "span_end", "lf_hit", "rf_hit"), got_new, got_old):
        assert np.array_equal(g, o), (name, np.nonzero(g != o)[0][:10], g[g != o][:10], o[g != o][:10])
    for name, g, r in zip(("span_start", "span_end", "lf_hit", "rf_hit"), got_new, ref):
        assert np.array_equal(g, r), (name, np.nonzero(g != r)[0][:10], g[g != r][:10], r[g != r][:10])
    win_new, redone_new, kern_new, fall_new = _debug_counts(err_new)
    win_old, redone_old, kern_old, fall_old = _debug_counts(err_old)
    print("windowed %d (old launch %d), redone %d (%d), kernels %s / %s, not taken %d" % (win_new, win_old, redone_new, redone_old, kern_new, kern_old, fall_new))
    assert kern_old == "lds" and fall_old == 0
    assert (win_new, redone_new) == (win_old, redone_old)
    return win_new, redone_new, kern_new, fall_new, got_new


# ---- the hand-made cases: (name, damaged flank, expected penalty or None, keyword arguments of _pair) ----
def _cases(rng):
    cases = []

    def add(name, flank, damaged, penalty=None, stands=None, **kw):
        cases.append(dict(name=name, flank=flank, damaged=damaged, penalty=penalty, stands=stands if stands is not None else (penalty is not None and penalty <= 15), kw=kw))

    f = _flank(rng)
    add("penalty 15: two substitutions and a deletion of six", f, _del(_sub(rng, f, [20, 200]), 100, 6), 15)
    f = _flank(rng)
    add("penalty 15: one substitution and an insertion of eight", f, _ins(rng, _sub(rng, f, [150]), 60, 8), 15)
    f = _flank(rng)
    add("penalty 16: three substitutions and an insertion of five", f, _ins(rng, _sub(rng, f, [20, 110, 200]), 60, 5), 16)
    f = _flank(rng)
    add("penalty 17: two substitutions and a deletion of eight", f, _del(_sub(rng, f, [20, 200]), 120, 8), 17)
    f = _flank(rng)
    add("penalty 17: one substitution and an insertion of ten", f, _ins(rng, _sub(rng, f, [30]), 140, 10), 17)
    f = _flank(rng)
    add("three substitutions and a gap of three", f, _del(_sub(rng, f, [15, 90, 170]), 130, 3), 14)
    f = _flank(rng)
    add("four substitutions and an inserted pair", f, _ins(rng, _sub(rng, f, [15, 90, 170, 240]), 50, 2), 15)
    f = _flank(rng)
    add("insertion run of ten (the bound G)", f, _ins(rng, f, 125, 10), 15)
    f = _flank(rng)
    add("deletion run of ten (the bound G)", f, _del(f, 125, 10), 15)
    f = _flank(rng)
    add("seeds spread over exactly twenty diagonals", f, _ins(rng, _ins(rng, f, 170, 10), 80, 10), 30)
    # windows clipped by the start of the read: fewer than `margin` = 25 bases in front of the piece (left side of the pair only: there
    # the damaged piece opens the read), and by its end (right side only)
    for n_head in (0, 3, 24):
        f = _flank(rng)
        add("window clipped at the start of the read (%d bases in front)" % n_head, f, _del(_sub(rng, f, [40]), 180, 2), 9, head=rand_dna(rng, n_head))
    for n_tail in (0, 4, 44):
        f = _flank(rng)
        add("window clipped at the end of the read (%d bases behind)" % n_tail, f, _ins(rng, _sub(rng, f, [222]), 70, 3), 10, tail=rand_dna(rng, n_tail))
    f = _flank(rng)
    add("start diagonals below zero: the read opens four bases inside the piece", f, _sub(rng, f, [60, 130, 210])[4:], 15, head=b"")
    # paths that cross from one diagonal to the next.  In window coordinates the piece's own diagonal is 25 (margin), raised by p when a
    # copy of the first segment's head sits p bases further left (a seed p diagonals lower widens the window); a gap behind the last
    # segment's head (position 235) moves the path without moving a seed.  Lane l holds the diagonals 2 l - 16 and 2 l - 15:
    #   25 -> 27 (insertion of two): lane 20 (high half) -> lane 21, its low and then its high half
    #   45 -> 48 (p = 20, insertion of three): lanes 30 -> 31 -> 32, the DPP row boundary;  44 -> 47 (p = 19): up to the boundary
    #   45 -> 42, 25 -> 23 (deletions): downwards
    #   15 -> 17 with a clipped window (15 bases in front): lanes 15 -> 16, another row boundary
    for p, g in ((0, 2), (20, 3), (19, 3), (20, -3), (0, -2), (13, 1)):
        f = _flank(rng)
        d = _sub(rng, f, [100])
        d = _ins(rng, d, 235, g) if g > 0 else _del(d, 235, -g)
        pre = f[:12] + rand_dna(rng, p - 12) if p else b""
        add("path crosses diagonals: window diagonal 25 + %d, gap of %+d behind the last seed" % (p, g), f, d, 7 + abs(g), pre=pre)
    f = _flank(rng)
    add("path crosses lanes 15 | 16 in a clipped window", f, _ins(rng, _sub(rng, f, [100]), 235, 2), 9, head=rand_dna(rng, 15))
    # repeats next to the gap: where the gap goes is the engine's tie-break
    for unit, n, gap in ((b"A", 14, -2), (b"A", 14, 3), (b"AC", 16, -2), (b"AC", 16, 2), (b"AC", 16, -3), (b"GT", 12, 4)):
        f = bytearray(_flank(rng))
        run = (unit * n)[:n]
        f[100:100 + n] = run
        f = bytes(f)
        d = _del(f, 104, -gap) if gap < 0 else _ins(rng, f, 104, gap, what=(unit * gap)[:gap])
        add("%s run of %d next to a gap of %+d" % (unit.decode(), n, gap), f, d, None, stands=True)
    # substitutions against gaps at equal penalty: six bases shifted by one (insertion + five matches + deletion = 12 = six substitutions);
    # count_matches() differs by five between the two
    for at in (60, 140):
        f = bytearray(_flank(rng))
        blk = bytearray(b"ACGTAC" if at == 60 else b"TGCATG")
        f[at:at + 6] = blk
        f[at - 1] = ord("G") if at == 60 else ord("A")
        f[at + 6] = ord("T") if at == 60 else ord("C")
        f = bytes(f)
        x = b"T" if at == 60 else b"C"
        d = f[:at] + x + bytes(blk[:5]) + f[at + 6:]
        add("substitutions against an insertion and a deletion at equal penalty (at %d)" % at, f, d, 12, tie=True)
    return cases


def _loci_of(rng, cases):
    loci, n_jobs = [], 0
    for c in cases:
        kw = {k: v for k, v in c["kw"].items() if k != "tie"}
        pair = _pair(c["flank"], c["damaged"], rng, **kw)
        if "head" in kw:
            pair = pair[:1]   # the piece at the start of the read: as left piece only
        elif "tail" in kw:
            pair = pair[1:]   # ... at its end: as right piece only
        loci += pair
        n_jobs += len(pair)
    return loci, n_jobs


def test_hand_made_cases_reach_the_window_launch_and_match(oracle, capfd):
    rng = np.random.default_rng(20261018)
    cases = _cases(rng)
    n_stand = 0
    for c in cases:  # the cases are what they say: penalty of the piece against the whole read, by the oracle
        kw = c["kw"]
        read = (kw["head"] if "head" in kw else rand_dna(rng, 200)) + kw.get("pre", b"") + c["damaged"] + (kw["tail"] if "tail" in kw else rand_dna(rng, 200))
        if c["penalty"] is not None:
            a = _penalty(oracle, c["flank"], read)
            assert abs(a["score"]) == c["penalty"], (c["name"], a["score"], oracle.cigar_string(a["ops"]))
    loci, n_jobs = _loci_of(rng, cases)
    for c in cases:
        n_stand += (1 if ("head" in c["kw"] or "tail" in c["kw"]) else 2) * bool(c["stands"])
    win, redone, kern, fall, got = _three_ways(oracle, capfd, loci)
    assert kern == "registers" and fall == 0
    assert win == n_jobs, (win, n_jobs)                      # every constructed piece ran on a window, nothing else did
    assert redone == n_jobs - n_stand, (redone, n_jobs - n_stand)  # ... and exactly the penalties above 15 were redone against the whole read
    assert (got[0] >= 0).all()  # every read spans: each alignment was accepted


def test_count_matches_of_the_tie_is_the_engines(oracle, capfd):
    """The co-optimal alignments of the tie cases differ in count_matches() by five: with the threshold just below the oracle's count the
    piece is a hit, just above it is none -- in all three."""
    rng = np.random.default_rng(7)
    cases = [c for c in _cases(rng) if c["kw"].get("tie")]
    assert len(cases) == 2
    for c in cases:
        read = rand_dna(rng, 200) + c["damaged"] + rand_dna(rng, 200)
        nm = _penalty(oracle, c["flank"], read)["n_match"]
        assert nm in (244, 249), nm
        loci, n_jobs = _loci_of(rng, [c])
        hits = []
        for frac in ((nm - 0.5) / F, (nm + 0.5) / F):
            win, redone, kern, fall, got = _three_ways(oracle, capfd, loci, frac=frac)
            assert kern == "registers" and fall == 0 and win == n_jobs and redone == 0
            hits.append((int(got[2][0]), int(got[3][2])))  # the damaged piece: left piece of locus 0's first read, right piece of locus 1's
        assert hits == [(2, 2), (0, 0)], (nm, hits)


@pytest.mark.parametrize("n_win", [0, 1, 3, 5])
def test_job_counts_around_the_claim_size(oracle, capfd, n_win):
    """Jobs are claimed four per atomic: lists of 0, 1, 3 and 5 alignments (an empty list, the tail of a claim, one claim and a bit)."""
    rng = np.random.default_rng(100 + n_win)
    f, o = _flank(rng), _flank(rng)
    tr = b"CAG" * 20
    reads = [rand_dna(rng, 150 + 7 * i) + _del(_sub(rng, f, [30 + i]), 100 + 9 * i, 2 + i % 3) + tr + o + rand_dna(rng, 150) for i in range(n_win)]
    reads += [rand_dna(rng, 140 + i) + f + tr + o + rand_dna(rng, 160) for i in range(3)]
    loci = [dict(left_flank=f, right_flank=o, tr=tr, motifs=[b"CAG"], ploidy=2, reads=reads)]
    win, redone, kern, fall, got = _three_ways(oracle, capfd, loci)
    assert kern == "registers" and fall == 0 and win == n_win and redone == 0
    assert (got[0] >= 0).all()


def _mutate(rng, seq, rate):
    """substitutions (half of the edits), insertions and deletions of one base (now and then two or three), `rate` edits per base"""
    out = bytearray(seq)
    for p in sorted((int(v) for v in rng.choice(len(seq), int(rng.binomial(len(seq), rate)), replace=False)), reverse=True):
        kind = int(rng.integers(0, 4))
        if kind < 2:
            out[p] = b"ACGT"[(b"ACGT".index(out[p]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 2:
            out[p:p] = rand_dna(rng, 1 if rng.random() < 0.8 else int(rng.integers(2, 4)))
        else:
            del out[p:p + (1 if rng.random() < 0.8 else int(rng.integers(2, 4)))]
    return bytes(out)


def _random_loci(rng, n_loci, reads_per_locus, rates=(0.01, 0.03)):
    loci = []
    for _ in range(n_loci):
        lf, rf = rand_dna(rng, F), rand_dna(rng, F)
        tr = b"CAG" * int(rng.integers(10, 40))
        reads = []
        for _ in range(reads_per_locus):
            rate = float(rng.uniform(*rates))
            l, r = _mutate(rng, lf, rate), _mutate(rng, rf, rate)
            reads.append(rand_dna(rng, int(rng.integers(60, 110))) + l + tr + r + rand_dna(rng, int(rng.integers(60, 110))))
        assert all(600 <= len(x) <= 900 for x in reads)
        loci.append(dict(left_flank=lf, right_flank=rf, tr=tr, motifs=[b"CAG"], ploidy=2, reads=reads))
    return loci


def test_random_reads_three_ways(oracle, capfd):
    """About 2 000 reads whose flanks carry substitutions and indels at 1 - 3 %: penalties on both sides of the bound."""
    rng = np.random.default_rng(424242)
    loci = _random_loci(rng, 100, 20)
    win, redone, kern, fall, got = _three_ways(oracle, capfd, loci)
    assert kern == "registers" and fall == 0
    assert win >= 1500 and 300 <= redone <= win - 300, (win, redone)


@pytest.mark.parametrize("segments", [4, 6])
def test_other_segment_counts(oracle, capfd, segments):
    """TRGT_WIN_SEGMENTS = 4 / 6 (developer build): bounds of 7 / 11 and narrower start ranges, the same kernel."""
    rng = np.random.default_rng(segments)
    loci = _random_loci(rng, 12, 20, rates=(0.004, 0.02))  # (penalties on both sides of the smaller bounds)
    win, redone, kern, fall, got = _three_ways(oracle, capfd, loci, env=dict(TRGT_WIN_SEGMENTS=segments))
    assert kern == "registers" and fall == 0 and win >= 100 and 10 <= redone <= win - 10, (win, redone)


def test_flank_beyond_the_staging_buffers_takes_the_lds_launch(oracle, capfd):
    """flank_len + 70 bases of window do not fit the kernel's 496-byte text buffer: the host plans the LDS launch for the whole call (the
    kernel's own fall-back is never entered), results as before."""
    rng = np.random.default_rng(99)
    n = 440
    lf, rf = rand_dna(rng, n), rand_dna(rng, n)
    tr = b"CAG" * 20
    reads = [rand_dna(rng, 20) + _del(_sub(rng, lf, [50 + i]), 200, 2) + tr + _ins(rng, _sub(rng, rf, [90]), 300 + i, 3) + rand_dna(rng, 20) for i in range(6)]
    reads.append(rand_dna(rng, 30) + lf + tr + rf + rand_dna(rng, 30))  # (all below the length from which reads take the long-read path)
    loci = [dict(left_flank=lf, right_flank=rf, tr=tr, motifs=[b"CAG"], ploidy=2, reads=reads)]
    win, redone, kern, fall, got = _three_ways(oracle, capfd, loci, flank_len=n)
    assert kern == "lds" and fall == 0 and win == 12
    assert (got[0] >= 0).all() and (got[2][:6] == 2).all() and (got[3][:6] == 2).all()
