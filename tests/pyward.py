"""Genotyper::Cluster restated from the reference alone (src/trgt/genotype/genotype_cluster.rs:58-227) and, for the linkage the reference
takes from kodama 0.3.0 (linkage(.., Method::Ward)), from the published definitions: Muellner's nearest-neighbour chain ("Modern hierarchical,
agglomerative clustering algorithms", 2011, fig. 3) and the Lance-Williams form of Ward's update.  Plain Python floats (IEEE f64, every
operation rounded once, nothing fused) and integer indices; nothing here is tuned for speed.  It is the third party between the oracle
(oracle/locus.cpp), the host path and the two device chains (trgt_amd/csrc/locus_cluster*.hpp), none of which it was written from.

kodama is not vendored and pinned by no data it produced, so the three choices a tie-heavy matrix exposes are parameters.  The defaults are
the project's reading; the other values are the altered readings tests/test_cluster_independent.py shows to be detected:
  ties          "first": among equal nearest neighbours the smallest index          "last": the largest
  lw_order      "reference": ((sx+sa) d_ax + (sx+sb) d_bx - sx d_ab) / (sa+sb+sx)   "alternate": the same sum taken in another order
  keep_previous True: a neighbour no closer than the previous chain element loses   False: it wins when it is exactly as close

`Counters` is filled while the restatement runs, so that a test can assert which decisions its input reached."""
import math
from fractions import Fraction

from pyconsensus import central_read  # genotype_cluster.rs:12-39, the reference's double loop  # noqa: F401  (re-exported)

MAX_OPS = 10000  # genotype_cluster.rs:236


class Counters:
    FIELDS = ("even_odd", "negative_cutoff", "outlier_redo", "dropped_tie", "dropped_no_tie", "swap", "chain_reentry", "tie_keeps_previous",
              "zero_merges")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}


def pair_index(n, i, j):
    """the condensed index of the pair i != j"""
    if i > j:
        i, j = j, i
    return n * i - i * (i + 3) // 2 + j - 1


def lance_williams(d_ax, d_bx, d_ab, sa, sb, sx, lw_order="reference"):
    """Ward's update of the squared distance from x to the merger of a and b (sizes as floats, as kodama converts them)"""
    sa, sb, sx = float(sa), float(sb), float(sx)
    if lw_order == "reference":
        return (((sx + sa) * d_ax) + ((sx + sb) * d_bx) - (sx * d_ab)) / (sa + sb + sx)
    if lw_order == "alternate":
        return (((sx + sa) * d_ax) - (sx * d_ab) + ((sx + sb) * d_bx)) / (sx + (sa + sb))
    raise ValueError(lw_order)


def linkage(dists, n, *, ties="first", lw_order="reference", keep_previous=True, counters=None):
    """dists: a list of n (n - 1) / 2 floats, squared and updated IN PLACE as the reference's matrix is.  Returns (steps, dists) with
    steps[i] = (cluster1, cluster2, dissimilarity, size) in SciPy's labelling."""
    assert len(dists) == n * (n - 1) // 2 and ties in ("first", "last")
    for p in range(len(dists)):
        dists[p] = dists[p] * dists[p]
    if n < 2:
        return [], dists
    active = [True] * n
    size = [1] * n
    chain = []
    merges = []  # (a, b, squared dissimilarity) in the order they are made, a < b

    def nearest(cur, prev):
        """the nearest active neighbour of cur and its squared distance; prev: the previous chain element (None: cur starts the chain)"""
        best_v, best_i, at_min = None, None, 0
        for i in range(n):  # the first (ties="last": the last) minimum in index order
            if i == cur or not active[i]:
                continue
            v = dists[pair_index(n, i, cur)]
            if best_v is None or v < best_v:
                best_v, best_i, at_min = v, i, 1
            elif v == best_v:
                at_min += 1
                if ties == "last":
                    best_i = i
        if prev is None:
            return best_i, best_v
        d_prev = dists[pair_index(n, prev, cur)]
        if best_v < d_prev or (best_v == d_prev and not keep_previous):
            return best_i, best_v
        if counters is not None and at_min > 1:
            counters.tie_keeps_previous += 1
        return prev, d_prev  # a neighbour that is no closer than the previous chain element does not replace it

    for _ in range(n - 1):
        if len(chain) <= 3:
            a = active.index(True)  # a new chain starts at the first active index
            chain = [a]
            b, best = nearest(a, None)
        else:
            if counters is not None:
                counters.chain_reentry += 1
            b = chain[-3]  # the merged pair leaves the chain, and so does the element before it: it is looked at again
            del chain[-3:]
            a = chain[-1]
        guard = 0
        while True:
            chain.append(b)
            nn, best = nearest(b, a)
            a, b = b, nn
            if b == chain[-2]:
                break
            guard += 1
            assert guard <= 2 * n, "the chain does not close"
        lo, hi = (a, b) if a < b else (b, a)
        if counters is not None and best == 0.0:
            counters.zero_merges += 1
        for x in range(n):
            if x == lo or x == hi or not active[x]:
                continue
            d_lo, p_hi = dists[pair_index(n, x, lo)], pair_index(n, x, hi)
            dists[p_hi] = lance_williams(d_lo, dists[p_hi], best, size[lo], size[hi], size[x], lw_order)  # the larger index survives
        size[hi] += size[lo]
        active[lo] = False
        merges.append((lo, hi, best))
    merges.sort(key=lambda m: m[2])  # list.sort is stable, as slice::sort_by is
    up = [-1] * (2 * n - 1)
    csize = [1] * n + [0] * (n - 1)
    steps = []
    for i, (p, q, d) in enumerate(merges):
        while up[p] >= 0:
            p = up[p]
        while up[q] >= 0:
            q = up[q]
        if p > q:
            p, q = q, p
        csize[n + i] = csize[p] + csize[q]
        up[p] = up[q] = n + i
        steps.append((p, q, math.sqrt(d), csize[n + i]))
    return steps, dists


def round_half_away(x):
    """f64::round"""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def cluster(dists, n, counters=None, **rules):
    """genotype_cluster.rs:154-227; dists is mutated"""
    assert n >= 2 and len(dists) == n * (n - 1) // 2
    if n == 2:
        return [[0], [1]]
    steps, _ = linkage(dists, n, counters=counters, **rules)

    def cluster_size(label):
        return 1 if label < n else steps[label - n][3]

    cutoff = 0.0
    min_cluster_size = max(2, round_half_away(0.01 * float(n)))
    for c1, c2, diss, _ in reversed(steps):
        if min(cluster_size(c1), cluster_size(c2)) >= min_cluster_size:
            cutoff = diss - 0.0001
            break
    if cutoff == 0.0:
        if counters is not None:
            counters.even_odd += 1
        return [list(range(0, n, 2)), list(range(1, n, 2))]
    if counters is not None and cutoff < 0.0:
        counters.negative_cutoff += 1
    num_groups = 0
    membership = [None] * (2 * n - 1)
    for cluster_index in range(len(steps) - 1, -1, -1):
        c1, c2, diss, _ = steps[cluster_index]
        label = cluster_index + n
        if diss <= cutoff:
            if membership[label] is None:
                membership[label] = num_groups
                num_groups += 1
            membership[c1] = membership[label]
            membership[c2] = membership[label]
    groups = []
    for g in membership[:n]:
        if g is not None:
            groups.append(g)
        else:
            groups.append(num_groups)
            num_groups += 1
    seqs_by_group = [[] for _ in range(num_groups)]
    for seq_index, g in enumerate(groups):
        seqs_by_group[g].append(seq_index)
    return seqs_by_group


def genotype_groups(groups):
    """:77-80: the stable sort_by_key(len) and two pop()s -- among groups of one size the later one first"""
    order = sorted(groups, key=len)
    return order[-1], order[-2]


def small_group_is_outlier(len1, len2, cov1, cov2):
    """:87-94"""
    return abs(len1 - len2) < 100 and min(cov1, cov2) * 4 < max(cov1, cov2)


def classify(n, group1, group2, len1, len2, dropped_dists=None, redo_lens=None, counters=None):
    """:95-151 behind the two consensus sequences.  len1 / len2: the lengths of the alleles of group1 / group2; redo_lens: those of the
    even / odd alleles, needed when small_group_is_outlier holds; dropped_dists[i] = (dist to allele 1, dist to allele 2) as get_dist gives
    them, for every read in neither group.  Returns (classification, redo)."""
    if small_group_is_outlier(len1, len2, len(group1), len(group2)):
        if counters is not None:
            counters.outlier_redo += 1
        e1, e2 = redo_lens
        cls = [i % 2 for i in range(n)]
        if e1 > e2:
            if counters is not None:
                counters.swap += 1
            cls = [1 - c for c in cls]
        return cls, True
    cls = [2] * n
    for i in group1:
        cls[i] = 0
    for i in group2:
        cls[i] = 1
    for i in range(n):
        tie_breaker = 1
        if cls[i] == 2:
            d1, d2 = dropped_dists[i]
            if d1 < d2:
                cls[i] = 0
            elif d2 < d1:
                cls[i] = 1
            else:
                tie_breaker = (tie_breaker + 1) % 2  # always 0: the variable is born in the loop
                cls[i] = tie_breaker
            if counters is not None:
                if d1 == d2:
                    counters.dropped_tie += 1
                else:
                    counters.dropped_no_tie += 1
    if len1 > len2:
        if counters is not None:
            counters.swap += 1
        cls = [1 - c for c in cls]
    return cls, False


def exact(k, n):
    """The primitive algorithm on the integer squared distances k (condensed), in exact arithmetic: merge the globally closest pair of
    clusters, update with the Lance-Williams formula, repeat.  Returns (merges, tie, min_gap): merges[i] = (frozenset of leaves,
    frozenset of leaves, exact squared height); tie: some step had two candidate pairs at exactly the smallest distance; min_gap: the smallest
    relative gap between the best and the second-best candidate over all steps (None when no step had two candidates)."""
    d = {}
    for i in range(n):
        for j in range(i + 1, n):
            d[(i, j)] = Fraction(int(k[pair_index(n, i, j)]))
    leaves = {i: frozenset([i]) for i in range(n)}
    merges, tie, min_gap = [], False, None
    key = lambda a, b: (a, b) if a < b else (b, a)
    while len(leaves) > 1:
        ranked = sorted(d.items(), key=lambda kv: kv[1])
        (a, b), best = ranked[0]
        if len(ranked) > 1:
            second = ranked[1][1]
            if second == best:
                tie = True
            gap = (second - best) / second if second != 0 else Fraction(0)
            min_gap = gap if min_gap is None or gap < min_gap else min_gap
        merges.append((leaves[a], leaves[b], best))
        sa, sb = len(leaves[a]), len(leaves[b])
        for x in leaves:
            if x == a or x == b:
                continue
            sx = len(leaves[x])
            d[key(b, x)] = ((sx + sa) * d[key(a, x)] + (sx + sb) * d[key(b, x)] - sx * best) / (sa + sb + sx)
            del d[key(a, x)]
        del d[(a, b)]
        leaves[b] = leaves[a] | leaves[b]
        del leaves[a]
    return merges, tie, min_gap
