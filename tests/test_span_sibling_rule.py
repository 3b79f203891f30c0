"""The sibling rule of the flank scan (trgt_amd/csrc/spans.hip, ScanArgs::min_matches), restated in Python and held against the oracle's
span location on synthetic reads.  No GPU.

The reference combines the two flank hits of a read as (lf.end, rf.start) and returns None when either is missing or lf.end > rf.start
(span_locater.rs:52-66).  With one piece found exactly and the other missed, the missed piece's alignment counts only inside the
admissible region Adm: [p0 + F, n) for a missed right piece (left exact at p0), [0, p1) for a missed left piece (right exact at p1).
The rule: no alignment is run where |Adm| < min_matches = ceil(F * min_flank_id_frac); such a read has no span.  Checked here: every
read the rule drops has span None in the oracle -- with cut points that sweep |Adm| across min_matches - 2 .. + 2 and across F, and with
a second copy of the missed piece (exact, and at 80-95 % identity) inside the inadmissible part of the read.
"""
import math

import numpy as np
import pytest

from oracle import binding as orc

F = 250
FRAC = 0.7
MIN_MATCHES = int(math.ceil(F * FRAC))  # 175
BASES = np.frombuffer(b"ACGT", np.uint8)


def admissible(read, lf_piece, rf_piece, flank_len):
    """(side of the missed piece, |Adm|) when exactly one piece is found exactly (leftmost occurrence), else None"""
    p0, p1 = read.find(lf_piece), read.find(rf_piece)
    if (p0 < 0) == (p1 < 0):
        return None
    return (1, len(read) - p0 - flank_len) if p1 < 0 else (0, p1)


def rule_drops(read, lf_piece, rf_piece, flank_len, min_matches):
    a = admissible(read, lf_piece, rf_piece, flank_len)
    return a is not None and a[1] < min_matches


def rnd(rng, n):
    return BASES[rng.integers(0, 4, size=n)].tobytes()


def degrade(rng, seq, identity):
    """substitutions, and a few one-base gaps, down to about `identity`"""
    a = bytearray(seq)
    for i in rng.choice(len(a), size=int(round(len(a) * (1.0 - identity))), replace=False):
        a[i] = int(BASES[(b"ACGT".index(a[i]) + int(rng.integers(1, 4))) % 4])
    out = bytes(a)
    for _ in range(int(rng.integers(0, 3))):
        i = int(rng.integers(1, len(out) - 1))
        out = out[:i] + (rnd(rng, 1) if rng.random() < 0.5 else b"") + out[i + int(rng.random() < 0.5):]
    return out


def make_reads(rng, lf, rf, n_reads):
    """truncated reads, both sides; returns (reads, kind): kind 'cut' plain, 'adv' with a copy of the missed piece in the inadmissible part"""
    sweep = [MIN_MATCHES + d for d in range(-2, 3)] + [F + d for d in range(-2, 3)]
    reads, kinds = [], []
    for i in range(n_reads):
        side = i & 1  # the missed piece: 1 right, 0 left
        # a third of the reads on the boundary values, the others anywhere from no room at all to well above the threshold
        adm = sweep[(i >> 1) % len(sweep)] if i % 3 == 0 else int(rng.integers(0, MIN_MATCHES + 40))
        tr = rnd(rng, int(rng.integers(0, min(adm, 60) + 1)))
        k = adm - len(tr)  # bases of the missed piece the read still holds (k >= F: the rest is context behind it -- then the piece is there, exactly)
        ctx = rnd(rng, int(rng.integers(0, 80)))
        adv = b""
        kind = "cut"
        if i % 4 == 3:  # a second copy of the missed piece, beyond the sibling
            kind = "adv"
            ident = 1.0 if i % 8 == 7 else float(rng.uniform(0.80, 0.95))
            adv = (rf if side else lf) if ident == 1.0 else degrade(rng, rf if side else lf, ident)
        if side:  # left context (+ copy of the right piece) + left piece + repeat + the first k bases of the right piece
            tail = rf[:k] if k <= F else rf + rnd(rng, k - F)
            read = ctx + adv + rnd(rng, int(rng.integers(0, 30))) + lf + tr + tail
        else:     # the last k bases of the left piece + repeat + right piece + (copy of the left piece) + right context
            head = lf[F - k:] if k <= F else rnd(rng, k - F) + lf
            read = head + tr + rf + rnd(rng, int(rng.integers(0, 30))) + adv + ctx
        reads.append(read)
        kinds.append(kind)
    return reads, kinds


def oracle_spans(lf, rf, reads, scoring):
    """find_tr_spans from the oracle's per-piece find_span: (lf.end, rf.start), None (-1) when either is missing or lf.end > rf.start"""
    thr = float(F) * FRAC
    ls, le, _, _ = orc.find_spans(lf, reads, *scoring, threshold=thr)
    rs, re_, _, _ = orc.find_spans(rf, reads, *scoring, threshold=thr)
    ok = (ls >= 0) & (rs >= 0) & (le <= rs)
    return np.where(ok, le, -1), np.where(ok, rs, -1)


N_LOCI, READS_PER_LOCUS = 40, 500  # 20 000 reads


@pytest.fixture(scope="module")
def census():
    rng = np.random.default_rng(20260117)
    rows = []  # (dropped, span is None, kind, side, |Adm| or None)
    for l in range(N_LOCI):
        lf, rf = rnd(rng, F), rnd(rng, F)
        reads, kinds = make_reads(rng, lf, rf, READS_PER_LOCUS)
        ss, _ = oracle_spans(lf, rf, reads, (2, 5, 1) if l % 2 == 0 else (1, 0, 1))
        for read, kind, s in zip(reads, kinds, ss):
            a = admissible(read, lf, rf, F)
            rows.append((rule_drops(read, lf, rf, F, MIN_MATCHES), int(s) < 0, kind, None if a is None else a[0], None if a is None else a[1]))
    return rows


def test_dropped_reads_have_no_span(census):
    assert len(census) >= 20000
    bad = [r for r in census if r[0] and not r[1]]
    assert not bad, bad[:5]


def test_rule_is_not_vacuous(census):
    dropped = sum(1 for r in census if r[0])
    print("dropped %d of %d truncated reads" % (dropped, len(census)))
    assert 3 * dropped >= len(census), (dropped, len(census))
    # every boundary value on either side, plain and adversarial, is among the inputs
    for side in (0, 1):
        for adm in [MIN_MATCHES + d for d in range(-2, 3)] + [F + d for d in range(-2, 3)]:
            hit = [r for r in census if r[3] == side and r[4] == adm]
            assert hit, (side, adm)
            assert all(r[0] == (adm < MIN_MATCHES) for r in hit)
    assert sum(1 for r in census if r[0] and r[2] == "adv") > 500


def test_bound_is_tight(census):
    """one base more room and the oracle does find spans: the rule could not ask for less than min_matches"""
    for side in (0, 1):
        assert any(not r[1] for r in census if r[3] == side and r[4] == MIN_MATCHES and r[2] == "cut"), side
