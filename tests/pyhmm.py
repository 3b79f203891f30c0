"""The reference's motif HMM restated in plain Python, from PacificBiosciences/trgt v3.0.0 `src/hmm/*.rs` and
`src/trgt/workflows/tr.rs:454-492` alone -- not from oracle/hmm.cpp, trgt_amd/hmm.py or the kernels.  It is the third party of
"oracle == restatement == GPU" (tests/test_hmm_independent.py, tests/test_hmm_independent_gpu.py).

Deliberately generic: a model is a number of states, five ln-emissions per state, and per state a LIST of incoming states with the ln
of their transition probabilities, in the order the builder gives them.  Nothing here knows about motif blocks, positions or lanes;
the column recursion walks the states in the order of `order_states` and the predecessors in list order, as hmm_model.rs does.

Arithmetic of the fill:
  "f64"    IEEE doubles; the sum is formed as (prev + ln p) + emission, the maximum is the FIRST STRICT one (hmm_model.rs:79-88)
  "exact"  every table entry taken as Fraction(float) (all of them dyadic, so the fill runs on integers over their common
           denominator): the true optimum of the model's own f64 tables, free of rounding
Exact ties (two predecessors whose f64 sums are equal and maximal) are counted: `Labelling.ties` over all filled cells,
`Labelling.path_ties` over the decisions the trace-back actually went through.

Standard library and numpy only; reads no file.
"""
import math
from fractions import Fraction

import numpy as np

NEG = float("-inf")
NAN = float("nan")
SENTINEL = ord("#")
CODE = {ord("#"): 0, ord("A"): 1, ord("T"): 2, ord("C"): 3, ord("G"): 4}  # encode_base, hmm_model.rs:243-252; anything else panics
LETTER = "#ATCG"

# HmmEvent, events.rs:5-15
MATCH, MISMATCH, INS, DEL, TRANS, SKIP, MOTIF_START, MOTIF_END = range(8)


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def ln(p):
    """f64::ln as set_trans / set_ems take it (hmm_model.rs:46, 51); ln(0) is -inf there, math.log raises instead"""
    return math.log(p) if p > 0.0 else NEG


class Block:  # HmmMotif, hmm_model.rs:21-26
    def __init__(self, first, last, motif_index):
        self.first, self.last, self.motif_index = first, last, motif_index


class Model:
    """Hmm, hmm_model.rs:12-19 and 28-52.  `ln_args` collects every probability whose ln was taken (for the table test)."""

    def __init__(self, n_states):  # Hmm::new, hmm_model.rs:29-42
        self.n = n_states
        self.em = [[NEG] * 5 for _ in range(n_states)]
        self.pred = [[] for _ in range(n_states)]
        self.lp = [[] for _ in range(n_states)]
        self.blocks = []
        self.ln_args = set()
        self._plan = self._quiet = None

    def trans(self, target, sources, probs):  # set_trans, hmm_model.rs:44-47
        assert len(sources) == len(probs)
        self.pred[target] = list(sources)
        self.lp[target] = [ln(p) for p in probs]
        self.ln_args.update(probs)

    def emit(self, target, probs):  # set_ems, hmm_model.rs:49-52
        assert len(probs) in (0, 5)
        self.em[target] = [ln(p) for p in probs]
        self.ln_args.update(probs)
        self._plan = self._quiet = None

    def silent(self, s):  # hmm_model.rs:62 and 211: no finite emission at all
        if self._quiet is None:
            self._quiet = [all(math.isinf(e) for e in row) for row in self.em]
        return self._quiet[s]

    def consumes(self, s):  # the test of traceback, hmm_model.rs:134
        return any(math.isfinite(e) for e in self.em[s])

    def emits_base(self, s):  # emits_base, hmm_model.rs:202-204: a finite emission for one of A T C G (the sentinel does not count)
        return any(math.isfinite(e) for e in self.em[s][1:])

    def visiting_order(self, by_index=False):
        """order_states, hmm_model.rs:206-240: emitting states by index, then the silent ones in rounds; a round takes, in index
        order, every remaining silent state none of whose predecessors is among the silent states remaining at the round's start"""
        loud = [s for s in range(self.n) if not self.silent(s)]
        quiet = [s for s in range(self.n) if self.silent(s)]
        if by_index:  # (not the reference: what a misreading would do; for the sensitivity check only)
            return loud + quiet
        placed = []
        while quiet:
            left = set(quiet)
            now = [s for s in quiet if not any(p in left for p in self.pred[s])]
            assert now, "silent states in a cycle"  # hmm_model.rs:234
            placed += now
            quiet = [s for s in quiet if s not in set(now)]
        return loud + placed


# ----------------------------------------------------------------------------------------------------------------- builder
def match_emissions(base):  # get_match_emissions, builder.rs:175-184
    if base == ord("N"):
        return [0.00, 0.25, 0.25, 0.25, 0.25]
    if base not in CODE or base == SENTINEL:
        raise ValueError("unknown motif base %r" % chr(base))
    row = [0.00, 0.03, 0.03, 0.03, 0.03]
    row[CODE[base]] = 0.90
    return row


def mismatch_seed(motif_len):  # builder.rs:93 (motif_len 1: a division by zero that no state ever uses)
    pairs = motif_len * (motif_len - 1)
    return 2.00 * (1.00 - 0.90) / float(pairs) if pairs else float("inf")


def motif_block(model, opening, motif):  # define_motif_block, builder.rs:80-173
    k = len(motif)
    match = [opening + 1 + i for i in range(k)]
    insert = [match[-1] + 1 + i for i in range(k)]
    delete = [insert[-1] + 1 + i for i in range(k - 1)]
    closing = opening + 3 * k  # builder.rs:149-150

    p_match = 0.90
    p_ins_stay = 0.25
    p_to_indel = (1.00 - p_match) / 2.00
    p_del_to_match = 0.50
    seed = mismatch_seed(k)

    for i, s in enumerate(match):  # builder.rs:94-120
        model.emit(s, match_emissions(motif[i]))
        if i == 0:
            model.trans(s, [opening], [p_match])
            continue
        p_mismatch = seed * float(k - i)
        sources = [s - 1, opening, insert[i - 1]]
        probs = [p_match, p_mismatch, 1.0 - p_ins_stay]
        if i >= 2:
            sources.append(delete[i - 2])
            probs.append(p_del_to_match)
        model.trans(s, sources, probs)

    for i, s in enumerate(insert):  # builder.rs:123-131
        model.emit(s, [0.00, 0.25, 0.25, 0.25, 0.25])
        model.trans(s, [s, match[i]], [p_ins_stay, p_to_indel])

    for i, s in enumerate(delete):  # builder.rs:134-147
        model.emit(s, [0.00] * 5)
        if i == 0:
            model.trans(s, [match[0]], [p_to_indel])
        else:
            model.trans(s, [match[i], delete[i - 1]], [p_to_indel, 1.0 - p_del_to_match])

    model.emit(closing, [0.00] * 5)  # builder.rs:151-172
    sources, probs = [match[-1], insert[-1]], [p_match, 1.0 - p_ins_stay]
    if delete:
        sources.append(delete[-1])
        probs.append(1.0)
    model.trans(closing, sources, probs)


def build(motifs):  # build_hmm, builder.rs:4-78
    motifs = [_b(m) for m in motifs]
    assert all(len(m) > 0 for m in motifs)
    n = 7 + sum(3 * len(m) + 1 for m in motifs)
    model = Model(n)
    model.motif_seqs = motifs
    first, last = 0, n - 1
    run_open, run_close = first + 1, last - 1

    model.emit(first, [1.00, 0.00, 0.00, 0.00, 0.00])
    model.emit(last, [1.00, 0.00, 0.00, 0.00, 0.00])
    model.trans(last, [run_close], [0.10])
    model.emit(run_open, [0.00] * 5)
    model.trans(run_open, [first, run_close], [1.00, 1.00])

    p_open, p_leave = 1.00, 0.50
    closings = []
    at = run_open + 1
    for m in motifs:  # builder.rs:26-37
        size = 3 * len(m) + 1
        closing = at + size - 1
        model.emit(at, [0.00] * 5)
        model.trans(at, [run_open, closing], [p_open, 1.0 - p_leave])
        motif_block(model, at, m)
        closings.append(closing)
        at += size
    assert at + 3 == run_close  # builder.rs:39

    skip, skip_close = at + 1, at + 2  # builder.rs:41-53
    model.emit(at, [0.00] * 5)
    model.trans(at, [run_open, skip_close], [p_open, 1.0 - p_leave])
    p_skip_stay = 0.5
    model.emit(skip, [0.00, 0.25, 0.25, 0.25, 0.25])
    model.trans(skip, [at, skip], [1.0, p_skip_stay])
    model.emit(skip_close, [0.00] * 5)
    model.trans(skip_close, [skip], [1.0 - p_skip_stay])
    closings.append(skip_close)

    model.emit(run_close, [0.00] * 5)  # builder.rs:55-57
    model.trans(run_close, list(closings), [p_leave] * (len(motifs) + 1))

    for i, m in enumerate(motifs):  # builder.rs:59-68
        model.blocks.append(Block(closings[i] - 3 * len(m), closings[i], i))
    model.blocks.append(Block(skip - 1, skip + 1, len(motifs)))  # builder.rs:70-75
    return model


# ------------------------------------------------------------------------------------------------------- Viterbi and trace-back
class Labelling:
    def __init__(self, path, score, ties, path_ties):
        self.path, self.score, self.ties, self.path_ties = path, score, ties, path_ties


def encode(query):  # hmm_model.rs:148-152: a sentinel in front and behind; any byte other than A T C G panics in the reference
    return [0] + [CODE[b] for b in _b(query)] + [0]


def _exact_tables(model):
    """every finite table entry as Fraction(float), then as an integer over the common (power-of-two) denominator"""
    den = 1
    for rows in (model.em, model.lp):
        for row in rows:
            for v in row:
                if math.isfinite(v):
                    den = max(den, Fraction(v).denominator)
    conv = lambda v: int(Fraction(v) * den) if math.isfinite(v) else NEG
    assert all(Fraction(conv(v), den) == Fraction(v) for rows in (model.em, model.lp) for row in rows for v in row if math.isfinite(v))
    return [[conv(v) for v in r] for r in model.em], [[conv(v) for v in r] for r in model.lp], den


def _cell(model, em, lp, zero, col_prev, col_now, s, symbol, at_first, strict=True):
    """calc_viterbi_score, hmm_model.rs:54-97, for one state and one column -> (score, predecessor or None, tie?)"""
    quiet = model.silent(s)
    term = zero if quiet else em[s][symbol]
    sources = model.pred[s]
    if at_first and sources and not quiet:  # hmm_model.rs:72-74
        return NEG, None, False
    col = col_now if quiet else col_prev  # lookback, hmm_model.rs:68 and 80
    best, who, tie = NEG, None, False
    for k, p in enumerate(sources):
        v = (col[p] + lp[s][k]) + term
        if (v > best) if strict else (v >= best and v != NEG):
            tie = (v == best)
            best, who = v, p
        elif v == best and v != NEG:
            tie = True
    if at_first and not sources and term != NEG:  # hmm_model.rs:91-94 (the start state)
        best, who, tie = term, s, False
    return best, who, tie


def _fill_scalar(model, symbols, exact, order=None, strict=True):
    """generate_mats, hmm_model.rs:99-114, cell by cell; floats, or integers over the tables' common denominator"""
    if exact:
        em, lp, den = _exact_tables(model)
        zero = 0
    else:
        em, lp, den, zero = model.em, model.lp, 1, 0.0
    order = order or model.visiting_order()
    back, tied, prev = [], [], None
    for i, sym in enumerate(symbols):
        now = [NEG] * model.n
        b, t = [None] * model.n, [False] * model.n
        for s in order:
            sc, who, tie = _cell(model, em, lp, zero, prev, now, s, sym, i == 0, strict)
            if who is not None:
                now[s], b[s], t[s] = sc, who, tie
        back.append(b)
        tied.append(t)
        prev = now
    return prev, back, tied, den


def _plan(model):
    """index arrays for the column-at-a-time f64 fill: the k-th listed predecessor of every emitting state, k = 0, 1, ..."""
    if model._plan is None:
        order = model.visiting_order()
        loud = [s for s in order if not model.silent(s)]
        quiet = [s for s in order if model.silent(s)]
        width = max([len(model.pred[s]) for s in loud] + [1])
        src = np.zeros((width, len(loud)), np.int64)
        lp = np.full((width, len(loud)), NEG)
        for j, s in enumerate(loud):
            for k, p in enumerate(model.pred[s]):
                src[k, j], lp[k, j] = p, model.lp[s][k]
        em = np.array([model.em[s] for s in loud]).T.copy()  # [symbol][emitting state]
        rootless = np.array([not model.pred[s] for s in loud])
        model._plan = (np.array(loud), src, lp, em, rootless, [(s, model.pred[s], model.lp[s]) for s in quiet])
    return model._plan


def _fill_columns(model, symbols):
    """generate_mats, hmm_model.rs:99-114, in f64.  Emitting states read the previous column only, so one column's worth of them is
    taken at once: for k = 0, 1, ... the k-th listed predecessor of every state is offered and accepted where strictly greater
    (the list order and the strict > of hmm_model.rs:79-88).  Silent states read the current column and go one by one."""
    loud, src, lp, em, rootless, quiet = _plan(model)
    back, tied = [], []
    prev = None
    for i, sym in enumerate(symbols):
        now = np.full(model.n, NEG)
        b = np.full(model.n, -1, np.int64)
        t = np.zeros(model.n, bool)
        if i == 0:  # hmm_model.rs:72-74 and 91-94
            ok = rootless & (em[sym] > NEG)
            now[loud[ok]] = em[sym][ok]
            b[loud[ok]] = loud[ok]
        else:
            best = np.full(len(loud), NEG)
            who = np.full(len(loud), -1, np.int64)
            tie = np.zeros(len(loud), bool)
            for k in range(src.shape[0]):
                v = (prev[src[k]] + lp[k]) + em[sym]
                up = v > best
                tie = (tie & ~up) | ((v == best) & (v > NEG))
                best = np.where(up, v, best)
                who = np.where(up, src[k], who)
            now[loud], b[loud], t[loud] = best, who, tie
        col = now.tolist()
        for s, sources, lps in quiet:
            bs, bw, bt = NEG, -1, False
            if i == 0 and not sources:  # hmm_model.rs:91-94 (no such state in a built model)
                bs, bw = 0.0, s
            for p, l in zip(sources, lps):
                v = (col[p] + l) + 0.0
                if v > bs:
                    bs, bw, bt = v, p, False
                elif v == bs and v != NEG:
                    bt = True
            if bw >= 0:
                col[s] = bs
                now[s], b[s], t[s] = bs, bw, bt
        back.append(b)
        tied.append(t)
        prev = now
    return prev, back, tied


def _walk_back(model, n_columns, back, tied):  # traceback, hmm_model.rs:125-142
    s, i = model.n - 1, n_columns - 1
    path, hits = [], 0
    while s != 0:
        path.append(s)
        hits += bool(tied[i][s])
        p = back[i][s]
        assert p is not None and p >= 0, "trace-back through a state without a score"
        if model.consumes(s):
            i -= 1
        s = int(p)
    path.append(0)
    path.reverse()
    return path, hits


def label(model, query, mode="f64", order=None, strict=True):
    """Hmm::label, hmm_model.rs:144-156 -> Labelling.  mode: "f64" (column at a time), "f64-scalar" (cell by cell), "exact".
    `order` / `strict` exist for the sensitivity check (a wrong visiting order, >= for >) and go through the scalar fill."""
    query = _b(query)
    if not query:
        return Labelling([], None, 0, 0)
    symbols = encode(query)
    if mode == "f64" and order is None and strict:
        last, back, tied = _fill_columns(model, symbols)
        score = float(last[model.n - 1])
        ties = int(sum(int(t.sum()) for t in tied))
    else:
        last, back, tied, den = _fill_scalar(model, symbols, mode == "exact", order, strict)
        score = Fraction(last[model.n - 1], den) if mode == "exact" else last[model.n - 1]
        ties = sum(sum(t) for t in tied)
    path, hits = _walk_back(model, len(symbols), back, tied)
    return Labelling(path, score, ties, hits)


def exact_path_score(model, query, path):
    """The exact sum (Fraction) of a given state path's terms over the model's f64 tables: per step the ln of the transition taken
    and, on an emitting state, the ln-emission of the query symbol it consumes.  Asserts that the path starts in state 0, ends in the
    last state, walks along existing edges only and consumes the whole query (both sentinels included)."""
    symbols = encode(query)
    path = [int(s) for s in path]
    assert path and path[0] == 0 and path[-1] == model.n - 1, "path does not run from the first to the last state"
    total, at = Fraction(0), 0
    for j, s in enumerate(path):
        if j:
            assert path[j - 1] in model.pred[s], "no edge %d -> %d" % (path[j - 1], s)
            total += Fraction(model.lp[s][model.pred[s].index(path[j - 1])])
        if not model.silent(s):
            assert at < len(symbols), "path consumes more than the query"
            e = model.em[s][symbols[at]]
            assert math.isfinite(e), "state %d cannot emit symbol %d" % (s, symbols[at])
            total += Fraction(e)
            at += 1
    assert at == len(symbols), "path consumes %d of %d symbols" % (at, len(symbols))
    return total


# ------------------------------------------------------------------------------------------------------------------ decoding
def label_motifs(model, path):  # Hmm::label_motifs, hmm_model.rs:158-200 -> [(motif_index, start, end)]
    opening = {b.first: i for i, b in enumerate(model.blocks)}
    spans, j = [], 0
    while j < len(path):
        s = path[j]
        if s not in opening:
            assert not model.emits_base(s)
            j += 1
            continue
        block = model.blocks[opening[s]]
        width = 0
        while path[j] != block.last:
            width += model.emits_base(path[j])
            j += 1
        while j < len(path) and path[j] == block.last:  # (the reference indexes past the end only if the path ends in a block)
            width += model.emits_base(path[j])
            j += 1
        begin = spans[-1][2] if spans else 0
        spans.append((opening[s], begin, begin + width))
    return spans


def base_match(model, s):  # get_base_match, events.rs:88-117 -> a byte
    row = model.em[s]
    assert len(row) == 5
    if not model.emits_base(s):
        return ord(" ")
    top = [i for i, e in enumerate(row) if e == max(row)]
    if len(top) == 1:
        return ord(LETTER[top[0]])
    return ord("N") if len(top) == 4 else ord(" ")


def events(model, path, query):  # get_events, events.rs:17-86
    query = _b(query)
    owner = [-1] * model.n
    for i, b in enumerate(model.blocks):
        for s in range(b.first, b.last + 1):
            owner[s] = i
    out, at = [], 0
    for j, s in enumerate(path):
        i = owner[s]
        if i == -1:
            out.append(TRANS)
            continue
        b = model.blocks[i]
        if s == b.first:
            out.append(MOTIF_START)
            out += [DEL] * (path[j + 1] - s - 1)
            continue
        if s == b.last:
            out.append(MOTIF_END)
            continue
        if i + 1 == len(model.blocks):
            out.append(SKIP)
            at += 1
            continue
        kind = (s - b.first - 1) // len(model.motif_seqs[b.motif_index])
        if kind == 0:
            want = base_match(model, s)
            ev = MATCH if (query[at] == want or want == ord("N")) else MISMATCH
        elif kind == 1:
            ev = INS
        else:
            assert kind == 2, "event decoding error"
            ev = DEL
        if ev in (MATCH, MISMATCH, INS, SKIP):
            at += 1
        out.append(ev)
    return out


def purity(model, path, query):  # calc_purity, purity.rs:6-41 -> (purity, edit distance, max distance)
    query = _b(query)
    if not query:
        return NAN, None, None
    ev = events(model, path, query)
    edit = sum(1 for e in ev if e in (DEL, INS, MISMATCH, SKIP))
    ref_len = sum(1 for e in ev if e in (MATCH, MISMATCH, DEL, SKIP))
    most = max(ref_len, len(query))
    return (float(most) - float(edit)) / float(most), edit, most


def remove_imperfect_motifs(model, path, query, max_motif_len=6):  # operations.rs:6-80
    query = _b(query)
    if not path:
        return []
    by_opening = {b.first: b for b in model.blocks}
    closings = {b.last for b in model.blocks}
    assert len(path) > 4
    out = [path[0], path[1]]
    run_close = model.n - 2
    j, at = 2, 0
    while j != len(path):
        assert path[j] in by_opening
        visit, seen = [], bytearray()
        while path[j] not in closings:
            visit.append(path[j])
            if model.emits_base(path[j]):
                seen.append(query[at])
                at += 1
            j += 1
        visit.append(path[j])
        j += 1
        b = by_opening[visit[0]]
        keep = True
        if b.motif_index + 1 != len(model.blocks) and (b.last - b.first) // 3 <= max_motif_len:
            motif = model.motif_seqs[b.motif_index]
            if len(seen) < len(motif):
                keep = False
            else:
                keep = all(want == ord("N") or got == want for want, got in zip(motif, seen))
        if keep:
            out += visit
        else:
            used = sum(1 for s in visit if model.emits_base(s))
            skip = model.blocks[-1]
            out += [skip.first] + [skip.first + 1] * used + [skip.last]
        if path[j] == run_close:
            out += path[j:j + 2]
            j += 2
    return out


# -------------------------------------------------------------------------------------------------------------------- utils
def replace_invalid_bases(seq, allowed):  # utils.rs:29-42
    seq, allowed = _b(seq), _b(allowed)
    return bytes(c if c in allowed else allowed[i % len(allowed)] for i, c in enumerate(seq))


def count_motifs(n_motifs, spans):  # utils.rs:3-9
    counts = [0] * n_motifs
    for m, _, _ in spans:
        counts[m] += 1
    return counts


def collapse_labels(spans):  # utils.rs:11-27
    out = []
    for m, s, e in spans:
        if out and out[-1][0] == m and out[-1][2] == s:
            out[-1] = (m, out[-1][1], e)
        else:
            out.append((m, s, e))
    return out


def clean_motifs(motifs):  # tr.rs:455-460
    return [replace_invalid_bases(m, b"ATCGN") for m in motifs]


def annotate(model, n_motifs, seq, mode="f64"):
    """the body of label_with_hmm's loop, tr.rs:464-489, on a model built from clean_motifs(...).  Returns a dict: path, spans (collapsed,
    skip spans dropped; [] where the reference has None), counts, purity, edit, maxd, and the Labelling (ties, score)."""
    seq = replace_invalid_bases(seq, b"ATCG")
    lab = label(model, seq, mode)
    pur, edit, most = purity(model, lab.path, seq)
    kept = [sp for sp in label_motifs(model, remove_imperfect_motifs(model, lab.path, seq, 6)) if sp[0] < n_motifs]
    return dict(seq=seq, path=lab.path, spans=collapse_labels(kept), counts=count_motifs(n_motifs, kept), purity=pur, edit=edit,
                maxd=most, labelling=lab)


def label_with_hmm(motifs, seqs, mode="f64"):  # tr.rs:454-492
    model = build(clean_motifs(motifs))
    return [annotate(model, len(motifs), s, mode) for s in seqs]
