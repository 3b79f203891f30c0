"""A restatement of what the wavefront aligner has to compute, written from the textbook definitions (Gotoh's recurrences with free
ends) and from the reference wrapper's own text -- wfaligner.rs:489-528 (the two spans and the four free-end arguments), :864-908
(get_alignment_span), :988-1000 (count_matches), :932-959 (the run-length CIGAR) and :534-593 (what an operation costs) -- and NOT
from oracle/wfa.cpp or anything under trgt_amd/csrc/.  There is no wavefront, diagonal, offset or heuristic in here: only tables over
(pattern position i, text position j).

    optimum()             the least penalty of an alignment, plain Python integers and lists: THE DEFINITION
    optimum_rows()        the same, one numpy row at a time (held to optimum() by tests/test_wfa_independent.py)
    check_alignment()     everything that can be said about a completed alignment without knowing how it was found
    check_score()         the same for score-only scope
    match_bracket()       the fewest and the most 'M' over all minimum-cost alignments of the flank configuration
    end_positions()       how many text positions an optimal flank alignment can end at
    placement_is_optimal  whether a placement of a piece in a read is one of the optimal ones

Conventions (wfaligner.rs:883-905): 'M' / 'X' consume one base of either sequence, 'I' one base of the TEXT, 'D' one of the PATTERN.
A gap of n bases costs n (indel, edit), g n (gap-linear), o + e n (gap-affine) or min(o1 + e1 n, o2 + e2 n) (two-piece); a
substitution costs 1 (edit), x (the rest) and is not allowed at all under the indel metric.  The aligner reports the penalty as it is
for indel and edit and NEGATED for the three gap metrics.

Free ends: an alignment may start at (0, j) with j <= tbf or at (i, 0) with i <= pbf, and may end at (|p|, j) with |t| - j <= tef or at
(i, |t|) with |p| - i <= pef; -1 stands for the sequence's length.  What lies beyond the allowance is paid as a gap.
"""
import numpy as np

METRICS = ("indel", "edit", "linear", "affine", "affine2p")
INF = 1 << 50
I32_MIN = -2147483648
KEY = 4096  # cost * KEY -/+ matches: one DP finds the most / the fewest matches among the minimum-cost alignments (matches < KEY)


def model(metric, pen=()):
    """(cost of a substitution or None, [(opening, extension) of each gap piece])"""
    if metric == "indel":
        return None, [(0, 1)]
    if metric == "edit":
        return 1, [(0, 1)]
    if metric == "linear":
        return pen[0], [(0, pen[1])]
    if metric == "affine":
        return pen[0], [(pen[1], pen[2])]
    if metric == "affine2p":
        return pen[0], [(pen[1], pen[2]), (pen[3], pen[4])]
    raise ValueError(metric)


def sign(metric):
    return 1 if metric in ("indel", "edit") else -1


def _free(span, pbf, pef, tbf, tef, n, m):
    if span == "end2end":
        return 0, 0, 0, 0
    cl = lambda v, L: L if v < 0 else min(v, L)
    return cl(pbf, n), cl(pef, n), cl(tbf, m), cl(tef, m)


def optimum(pattern, text, metric, pen=(), span="end2end", pbf=0, pef=0, tbf=0, tef=0):
    """The least penalty.  Three kinds of cell value per (i, j): the best alignment of any kind that ends here (M), the best that ends in
    an inserted text base paid by gap piece k (I[k]), the best that ends in a deleted pattern base (D[k])."""
    p, t = bytes(pattern), bytes(text)
    n, m = len(p), len(t)
    x, pieces = model(metric, pen)
    pbf, pef, tbf, tef = _free(span, pbf, pef, tbf, tef, n, m)
    K = range(len(pieces))
    M = [[INF] * (m + 1) for _ in range(n + 1)]
    I = [[[INF] * (m + 1) for _ in range(n + 1)] for _ in K]
    D = [[[INF] * (m + 1) for _ in range(n + 1)] for _ in K]
    for i in range(n + 1):
        for j in range(m + 1):
            best = INF
            if (i == 0 and j <= tbf) or (j == 0 and i <= pbf):
                best = 0                                     # a free start
            if i > 0 and j > 0:
                if p[i - 1] == t[j - 1]:
                    best = min(best, M[i - 1][j - 1])
                elif x is not None:
                    best = min(best, M[i - 1][j - 1] + x)
            for k in K:
                o, e = pieces[k]
                if j > 0:
                    I[k][i][j] = min(M[i][j - 1] + o + e, I[k][i][j - 1] + e)
                    best = min(best, I[k][i][j])
                if i > 0:
                    D[k][i][j] = min(M[i - 1][j] + o + e, D[k][i - 1][j] + e)
                    best = min(best, D[k][i][j])
            M[i][j] = best
    ends = [M[n][j] for j in range(m - tef, m + 1)] + [M[i][m] for i in range(n - pef, n + 1)]
    return min(ends)


def _rows(p, t, match, mism, pieces, pbf, pef, tbf, tef):
    """Row-vectorised form of the table above with a cost for a match as well.  Returns (M of the last row, M of the last column).
    The insertion state of a row is a prefix minimum over the cells of that row that are NOT themselves insertions:
    min over j' < j of base[j'] + o + e (j - j') -- exact, because opening a gap from a cell that is itself an insertion (+ o + e)
    never beats extending it (+ e), o being >= 0."""
    n, m = len(p), len(t)
    tt = np.frombuffer(t, np.uint8) if m else np.zeros(0, np.uint8)
    j = np.arange(m + 1, dtype=np.int64)

    def close(base):
        M = base.copy()
        for o, e in pieces:
            run = np.minimum.accumulate(base - e * j)
            ins = np.full(m + 1, INF, np.int64)
            ins[1:] = run[:-1] + o + e * j[1:]
            M = np.minimum(M, ins)
        return np.minimum(M, INF)

    M = close(np.where(j <= tbf, 0, INF).astype(np.int64))
    D = [np.full(m + 1, INF, np.int64) for _ in pieces]
    last_col = [int(M[m])]
    for i in range(1, n + 1):
        base = np.full(m + 1, INF, np.int64)
        if m:
            eq = tt == p[i - 1]
            base[1:] = M[:-1] + np.where(eq, match, INF if mism is None else mism)
        for k, (o, e) in enumerate(pieces):
            D[k] = np.minimum(np.minimum(M + (o + e), D[k] + e), INF)
            base = np.minimum(base, D[k])
        if i <= pbf:
            base[0] = min(int(base[0]), 0)
        M = close(np.minimum(base, INF))
        last_col.append(int(M[m]))
    return M, last_col


def optimum_rows(pattern, text, metric, pen=(), span="end2end", pbf=0, pef=0, tbf=0, tef=0):
    p, t = bytes(pattern), bytes(text)
    n, m = len(p), len(t)
    x, pieces = model(metric, pen)
    pbf, pef, tbf, tef = _free(span, pbf, pef, tbf, tef, n, m)
    last_row, last_col = _rows(p, t, 0, x, pieces, pbf, pef, tbf, tef)
    return min(int(last_row[m - tef:].min()), min(last_col[n - pef:]))


def match_bracket(piece, read, x=2, o=5, e=1):
    """(optimum, fewest matches, most matches) over all minimum-cost alignments of align_ends_free(piece, 0, 0, read, |read|, |read|),
    gap-affine: one DP each on the key cost * KEY + matches and cost * KEY - matches."""
    p, t = bytes(piece), bytes(read)
    assert len(p) < KEY
    m = len(t)
    lo_row, _ = _rows(p, t, 1, x * KEY, [(o * KEY, e * KEY)], 0, 0, m, m)
    hi_row, _ = _rows(p, t, -1, x * KEY, [(o * KEY, e * KEY)], 0, 0, m, m)
    k_lo, k_hi = int(lo_row.min()), int(hi_row.min())
    cost = k_lo // KEY
    assert (k_hi + KEY - 1) // KEY == cost, (k_lo, k_hi)
    return cost, k_lo - cost * KEY, cost * KEY - k_hi


def end_positions(piece, read, x=2, o=5, e=1):
    """(optimum, the number of text positions at which a minimum-cost alignment of the flank configuration can end)"""
    p, t = bytes(piece), bytes(read)
    row, _ = _rows(p, t, 0, x, [(o, e)], 0, 0, len(t), len(t))
    best = int(row.min())
    return best, int((row == best).sum())


def placement_is_optimal(piece, read, ts, te, x=2, o=5, e=1):
    """Is there a minimum-cost alignment of the flank configuration that begins at text position ts and ends at te (get_alignment_span's
    text span: free leading and trailing text bases are outside it)?  None for an end that is not known: any will do.  (Which of
    several optimal placements an aligner reports is a tie-break that nothing pins.)"""
    lo, hi = 0 if ts is None else ts, len(read) if te is None else te
    if not (0 <= lo <= hi <= len(read)):
        return False
    here = optimum_rows(piece, read[lo:hi], "affine", (x, o, e), "endsfree", 0, 0, -1 if ts is None else 0, -1 if te is None else 0)
    return here == optimum_rows(piece, read, "affine", (x, o, e), "endsfree", 0, 0, -1, -1)


# ---------------------------------------------------------------------------------------------------------------- the checker
class Rejected(AssertionError):
    """check_alignment's verdict; .clause names the property that does not hold"""

    def __init__(self, clause, detail=""):
        AssertionError.__init__(self, "%s: %s" % (clause, detail))
        self.clause = clause


def gap_cost(metric, pen, n):  # wfaligner.rs:534-593
    _, pieces = model(metric, pen)
    return min(o + e * n for o, e in pieces)


def runs_of(ops):
    out = []
    for c in ops:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return out


def run_length_cigar(ops):  # wfaligner.rs:932-959 with show_mismatches: '=' 7, 'X' 8, 'I' 1, 'D' 2; length in the upper 28 bits
    code = {"M": 7, "X": 8, "I": 1, "D": 2}
    return [(n << 4) | code[c] for c, n in runs_of(ops)]


def expand_cigar(cigar):
    out = []
    for w in cigar:
        w = int(w)
        c = {7: "M", 8: "X", 1: "I", 2: "D"}.get(w & 15)
        if c is None or (w >> 4) == 0:
            raise Rejected("cigar", "word %#x is no run of = X I D" % w)
        if out and out[-1][-1] == c:
            raise Rejected("cigar", "two adjacent runs of %s" % c)
        out.append(c * (w >> 4))
    return "".join(out)


def alignment_span(ops, span, n, m):  # wfaligner.rs:864-908
    if span == "end2end":
        return [0, n, 0, m]
    i = j = 0
    ps = pe = ts = te = 0
    started = False
    for c in ops:
        if c == "I":
            j += 1
        elif c == "D":
            i += 1
        else:
            if not started:
                ps, ts, started = i, j, True
            i += 1
            j += 1
            pe, te = i, j
    return [ps, pe, ts, te]


def penalty_of(ops, metric, pen, pbf, pef, tbf, tef):
    """what the operations cost: a leading run of up to tbf inserted (or pbf deleted) bases and a trailing run of up to tef inserted (or
    pef deleted) bases are free, the rest of such a run is a gap like any other"""
    x, _ = model(metric, pen)
    r = runs_of(ops)
    if r:
        r[0][1] -= min(r[0][1], {"I": tbf, "D": pbf}.get(r[0][0], 0))
    if r:
        r[-1][1] -= min(r[-1][1], {"I": tef, "D": pef}.get(r[-1][0], 0))
    total = 0
    for c, k in r:
        if k == 0 or c == "M":
            continue
        if c == "X":
            if x is None:
                raise Rejected("bases", "a substitution under the indel metric")
            total += x * k
        else:
            total += gap_cost(metric, pen, k)
    return total


def check_alignment(pattern, text, metric, pen, span, free, result, exact, best=None, score_may_be_unset=False, score_is_a_bound=False):
    """result: dict(score, n_match, span4, cigar, ops) of a job with status 0 -- ops the expanded operations as str / bytes, or None when
    they were not asked for (then the run-length CIGAR alone is taken apart).  free = (pbf, pef, tbf, tef).  exact: the aligner ran
    with Heuristic::None.  best: optimum() of the pair, None when it is beyond the budget (the optimum clause is skipped then).
    score_may_be_unset: the one documented exception -- a BiWFA alignment that took the unidirectional base case never sets cigar.score.
    score_is_a_bound: BiWFA under a heuristic reports the penalty its top-level breakpoint promised, and the halves, aligned again under
    the same heuristic, need not keep that promise: the score has the right sign and is no better than the optimum, and that is all.
    Raises Rejected(clause); returns the penalty of the operations."""
    p, t = bytes(pattern), bytes(text)
    n, m = len(p), len(t)
    pbf, pef, tbf, tef = _free(span, *free, n, m)
    cigar = [int(w) for w in result["cigar"]]
    if result.get("ops") is None:
        ops = expand_cigar(cigar)
    else:
        ops = result["ops"] if isinstance(result["ops"], str) else bytes(result["ops"]).decode()
    i = j = matches = 0
    for k, c in enumerate(ops):
        if c in "MX":
            if i >= n or j >= m:
                raise Rejected("consumes", "operation %d runs past a sequence" % k)
            if (p[i] == t[j]) != (c == "M"):
                raise Rejected("bases", "%s at pattern %d / text %d" % (c, i, j))
            matches += c == "M"
            i += 1
            j += 1
        elif c == "I":
            j += 1
        elif c == "D":
            i += 1
        else:
            raise Rejected("consumes", "operation %r" % c)
    if (i, j) != (n, m):
        raise Rejected("consumes", "operations cover %d / %d of %d / %d bases" % (i, j, n, m))
    if int(result["n_match"]) != matches:
        raise Rejected("n_match", "%d reported, %d 'M'" % (result["n_match"], matches))
    if cigar != run_length_cigar(ops):
        raise Rejected("cigar", "not the run-length form of the operations")
    want = alignment_span(ops, span, n, m)
    if [int(v) for v in result["span4"]] != want:
        raise Rejected("span", "%s reported, %s by the operations" % (list(result["span4"]), want))
    cost = penalty_of(ops, metric, pen, pbf, pef, tbf, tef)
    score = int(result["score"])
    if score_is_a_bound and not score_may_be_unset:
        if score != 0 and (score > 0) != (sign(metric) > 0):
            raise Rejected("sign", "%d reported for metric %s" % (score, metric))
        if best is not None and abs(score) < best:
            raise Rejected("score", "%d reported, below the optimum %d" % (score, best))
    elif not score_may_be_unset:
        if abs(score) != cost:
            raise Rejected("score", "%d reported, the operations cost %d" % (score, cost))
        if score != sign(metric) * cost:
            raise Rejected("sign", "%d reported for metric %s" % (score, metric))
    if best is not None:
        if cost < best:
            raise Rejected("optimum", "operations cost %d, below the plain-DP optimum %d: the restatement is wrong" % (cost, best))
        if exact and cost != best:
            raise Rejected("optimum", "operations cost %d, the optimum is %d" % (cost, best))
    return cost


def check_score(score, metric, exact, best):
    """score-only scope: +-optimum with Heuristic::None, no better than it otherwise"""
    score = int(score)
    if score != 0 and (score > 0) != (sign(metric) > 0):
        raise Rejected("sign", "%d reported for metric %s" % (score, metric))
    if exact and abs(score) != best:
        raise Rejected("optimum", "%d reported, the optimum is %d" % (score, best))
    if abs(score) < best:
        raise Rejected("optimum", "%d reported, below the optimum %d" % (score, best))
