"""repair_consensus / central_read / make_consensus restated from the reference alone (src/trgt/genotype/consensus.rs:5-111,
genotype_cluster.rs:12-56), in plain Python lists and str: the third party between the oracle (oracle/locus.cpp) and the device
kernel (trgt_amd/csrc/consensus_vote.hpp), which were written by one hand.  Nothing here is tuned for speed.

A CIGAR is a list of (len, op) with op one of "=", "M", "X", "D", "I" (the run-length form utils::align hands over).  `Counters`
is filled while the restatement runs: tests/test_consensus_cases.py asserts from it that the seeded lists reach the decisions they
are meant to reach."""

BASES = "ATCG"  # consensus.rs:6 -- the counter order is A, T, C, G, deleted


class Counters:
    FIELDS = ("vote_ties", "deleted_wins", "ins_candidates", "ins_taken", "ins_exactly_half", "count_eq_without", "string_ties",
              "trailing_ins_groups")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}


def _base_index(b):
    if b not in BASES:
        raise ValueError("Encountered unexpected base %r" % b)  # consensus.rs:81
    return BASES.index(b)


def get_ins_consensus(ins_by_read, num_reads, counters=None):
    """consensus.rs:94-111: sort, group equal strings, stable sort by descending count, the first one -- taken only when more reads
    carry it than carry no insertion here"""
    ins = sorted(ins_by_read)  # str order = byte order for ASCII = Rust's String order
    without = num_reads - len(ins)
    groups = []  # chunk_by: (string, count) in sorted order
    for s in ins:
        if groups and groups[-1][0] == s:
            groups[-1][1] += 1
        else:
            groups.append([s, 1])
    ranked = sorted(groups, key=lambda g: -g[1])  # sorted() is stable, as Itertools::sorted_by is
    top, count = ranked[0]
    if counters is not None:
        if count == without:
            counters.count_eq_without += 1
        if len(ranked) > 1 and ranked[1][1] == count:
            counters.string_ties += 1
    return top if count > without else ""


def repair_consensus(reference, seqs, aligns, counters=None):
    """consensus.rs:5-72"""
    n_ref = len(reference)
    ref_counts = [[0, 0, 0, 0, 0] for _ in range(n_ref)]
    ref_inserts = [[] for _ in range(n_ref + 1)]
    for seq_index, operations in enumerate(aligns):
        seq = seqs[seq_index]
        x = y = 0
        for op_len, op in operations:
            if op in ("=", "M", "X"):
                piece = seq[x:x + op_len]
                assert len(piece) == op_len, "CIGAR runs past the member"
                for k, b in enumerate(piece):
                    ref_counts[y + k][_base_index(b)] += 1  # IndexError past the backbone, as the reference panics
                x += op_len
                y += op_len
            elif op == "D":
                for k in range(op_len):
                    ref_counts[y + k][4] += 1
                y += op_len
            elif op == "I":
                piece = seq[x:x + op_len]
                assert len(piece) == op_len, "CIGAR runs past the member"
                ref_inserts[y].append(piece)
                x += op_len
            else:
                raise ValueError("Unexpected CIGAR operation: %r" % (op,))
        if operations:  # (a member whose alignment failed has no runs: it is counted in len(seqs) and casts no vote)
            assert x == len(seq) and y == n_ref, "CIGAR does not end at the ends of member %d: x %d of %d, y %d of %d" % (
                seq_index, x, len(seq), y, n_ref)
    consensus_indexes = []
    for rec in ref_counts:
        best = 0
        for i in range(5):
            if rec[i] >= rec[best]:  # Iterator::max_by_key returns the LAST maximum
                best = i
        consensus_indexes.append(best)
        if counters is not None:
            top = max(rec)
            if top > 0 and sum(1 for v in rec if v == top) >= 2:
                counters.vote_ties += 1
            if best == 4:
                counters.deleted_wins += 1
    n = len(seqs)
    consensus = []
    for ref_pos, base_index in enumerate(consensus_indexes):
        ins = ref_inserts[ref_pos]
        if counters is not None and ins and len(ins) == n // 2:
            counters.ins_exactly_half += 1
        if len(ins) > n // 2:
            taken = get_ins_consensus(ins, n, counters)
            if counters is not None:
                counters.ins_candidates += 1
                if taken:
                    counters.ins_taken += 1
            consensus.append(taken)
        if base_index != 4:
            consensus.append(BASES[base_index])
    if counters is not None and ref_inserts[n_ref]:  # never looked at by the loop above
        counters.trailing_ins_groups += 1
    return "".join(consensus)


def central_read(num_seqs, group, dists):
    """genotype_cluster.rs:12-39"""
    group_size = len(group)
    if group_size <= 2:
        return group[0]
    dist_sums = [0.0] * group_size
    for i in range(group_size - 1):
        for j in range(i + 1, group_size):
            index1, index2 = group[i], group[j]
            mat_index = num_seqs * index1 - index1 * (index1 + 3) // 2 + index2 - 1
            dist_sums[i] += dists[mat_index]
            dist_sums[j] += dists[mat_index]
    best = 0
    for i in range(1, group_size):
        if dist_sums[i] < dist_sums[best]:  # Iterator::min_by returns the FIRST minimum
            best = i
    return group[best]


def make_consensus(num_seqs, trs, dists, group, align, counters=None):
    """genotype_cluster.rs:41-56 without the TrSize: align(backbone, seqs) -> one CIGAR per member (utils::align)"""
    seqs = [trs[i] for i in group]
    backbone = trs[central_read(num_seqs, group, dists)]
    aligns = align(backbone, seqs)
    return repair_consensus(backbone, seqs, aligns, counters)
