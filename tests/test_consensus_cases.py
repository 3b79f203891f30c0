"""repair_consensus (consensus.rs:5-111) on hand-built CIGAR groups, without a GPU: the restatement written from the reference alone
(tests/pyconsensus.py) gives the consensus each hand-made vector states literally, the oracle's repair_consensus (oracle/locus.cpp,
through orc_repair_consensus) gives what the restatement gives on every hand-made, shape and random group, and the oracle's whole-locus
result on the designed haploid cluster loci is the restatement's make_consensus over the oracle's own alignments.  The device kernel
meets the same groups in tests/test_consensus_vote_gpu.py.

A one-line change of a decision in the oracle's repair_consensus fails here: `>=` to `>` in the winner loop, `top_count > without` to
`>=`, `j - i > top_count` to `>=` and a dropped `x += n` of an insertion each fail test_hand_vectors_oracle (and the random lists).
`> seqs.size() / 2` to `>=` cannot fail any test: with exactly n / 2 insertions, n - n / 2 >= n / 2 members are without one, so no string's
count can exceed them and nothing is emitted either way -- the condition only spares the work."""
import numpy as np
import pytest

import consensus_cases as cases
import pyconsensus

# floors of the restatement's counters on every random list (they keep the comparisons from passing on inputs that decide nothing)
FLOORS = dict(vote_ties=100, ins_candidates=100, ins_taken=50, ins_exactly_half=50, count_eq_without=20, string_ties=20, trailing_ins_groups=10)
DIFFERS_FLOOR = 200


def restate(backbone, members, counters=None):
    return pyconsensus.repair_consensus(backbone, [m for m, _ in members], [ops for _, ops in members], counters)


def by_oracle(oracle, backbone, members):
    return oracle.repair_consensus(backbone, [m for m, _ in members], [cases.words(ops) for _, ops in members]).decode()


@pytest.fixture(scope="module")
def random_lists():
    return {seed: cases.random_groups(seed) for seed in cases.RANDOM_SEEDS}


@pytest.mark.parametrize("name,backbone,members,expected", cases.HAND, ids=[h[0] for h in cases.HAND])
def test_hand_vectors_restatement(name, backbone, members, expected):
    assert restate(backbone, members) == expected


def test_hand_vectors_oracle(oracle):
    for name, backbone, members, expected in cases.HAND:
        assert by_oracle(oracle, backbone, members) == expected, name


def test_shape_vectors(oracle):
    for name, backbone, members, expected in cases.SHAPES:
        assert restate(backbone, members) == expected, name
        assert by_oracle(oracle, backbone, members) == expected, name


def test_unknown_op_is_an_error():
    with pytest.raises(ValueError):
        restate("AC", [("AC", [(1, "="), (1, "N")])])
    with pytest.raises(ValueError):
        restate("AC", [("AN", [(2, "=")])])


@pytest.mark.parametrize("seed", cases.RANDOM_SEEDS)
def test_random_lists(oracle, random_lists, seed):
    groups = random_lists[seed]
    assert len(groups) == 300
    counters = pyconsensus.Counters()
    differs = 0
    for g, (backbone, members) in enumerate(groups):
        assert 1 <= len(backbone) <= 80 and 1 <= len(members) <= 12
        for member, ops in members:
            assert set(member) <= set("ACGT") and all(a[1] != b[1] for a, b in zip(ops, ops[1:])), g
        want = restate(backbone, members, counters)  # (asserts that every CIGAR ends at both sequences' ends)
        assert by_oracle(oracle, backbone, members) == want, (seed, g)
        differs += want != backbone
    print("seed %d: %s, consensus differs from the backbone in %d of 300" % (seed, counters.as_dict(), differs))
    for name, floor in FLOORS.items():
        assert getattr(counters, name) >= floor, (name, getattr(counters, name), floor)
    assert differs >= DIFFERS_FLOOR, differs


# ---------------------------------------------------------------------------------------------------------------- designed loci
MAX_OPS = 10000  # genotype_cluster.rs:236


def _batch(pairs):
    """oracle.wfa_batch layout of (pattern, text) pairs"""
    pats, txts = [p for p, _ in pairs], [t for _, t in pairs]
    plen, tlen = np.array([len(p) for p in pats], np.uint32), np.array([len(t) for t in txts], np.uint32)
    blob = ("".join(pats) + "".join(txts)).encode()
    pat_off = np.concatenate([[0], np.cumsum(plen[:-1], dtype=np.uint64)]).astype(np.uint64)
    txt_off = (np.concatenate([[0], np.cumsum(tlen[:-1], dtype=np.uint64)]) + int(plen.sum())).astype(np.uint64)
    off = np.zeros(len(pairs) + 1, np.uint64)
    off[1:] = np.cumsum(plen.astype(np.uint64) + tlen.astype(np.uint64) + 1)
    return dict(seqs=np.frombuffer(blob, np.uint8).copy(), pat_off=pat_off, pat_len=plen, txt_off=txt_off, txt_len=tlen, cigar_off=off, ops_off=off)


def oracle_dists(oracle, trs):
    """get_dist_matrix (genotype_cluster.rs:238-286): score-only BiWFA, edit; sqrt(|length difference|) beyond MAX_OPS"""
    pairs = [(i, j) for i in range(len(trs)) for j in range(i + 1, len(trs))]
    todo = [(i, j) for i, j in pairs if len(trs[i]) * len(trs[j]) <= MAX_OPS]
    score = {}
    if todo:
        p = oracle.wfa_params(metric="edit", scope="score", memory="ultralow")
        r = oracle.wfa_batch(p, _batch([(trs[i], trs[j]) for i, j in todo]), want_ops=False)
        assert (r["status"] == 0).all()
        score = {ij: abs(int(s)) for ij, s in zip(todo, r["score"])}
    return [float(np.sqrt(float(score[ij] if ij in score else abs(len(trs[ij[0]]) - len(trs[ij[1]]))))) for ij in pairs]


def oracle_align(oracle):
    """utils::align (align.rs:14-28): BiWFA, gap-affine 2,5,1, the backbone as pattern; the run-length CIGAR with = and X"""
    def align(backbone, seqs):
        p = oracle.wfa_params(metric="affine", x=2, o1=5, e1=1, scope="alignment", memory="ultralow")
        r = oracle.wfa_batch(p, _batch([(backbone, s) for s in seqs]), want_ops=False)
        off = _batch([(backbone, s) for s in seqs])["cigar_off"]
        return [[(int(w) >> 4, "MIDNSHP=X"[int(w) & 0xF]) for w in r["cigar"][int(off[k]):int(off[k]) + int(r["cigar_len"][k])]]
                for k in range(len(seqs))]
    return align


def test_designed_loci_oracle(oracle):
    for k, L in enumerate(cases.designed_loci()):
        ref = oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], max_depth=10000, ploidy=1, genotyper=1)
        kept = [int(r) for r in ref["kept_read"]]
        assert sorted(kept) == list(range(L["depth"])), k  # every read spans: every segment votes
        for r in kept:
            assert L["reads"][r][int(ref["span_start"][r]):int(ref["span_end"][r])].decode() == L["segments"][r], (k, r)
        trs = [L["segments"][r] for r in kept]
        dists = oracle_dists(oracle, trs)
        if L["long"]:
            assert ref["stats"]["n_wfa_ed"] == 0
        counters = pyconsensus.Counters()
        want = pyconsensus.make_consensus(len(trs), trs, dists, list(range(len(trs))), oracle_align(oracle), counters)
        assert ref["alleles"] == [want], k
        if L["depth"] == 300:  # (the deep locus leaves the vote something to repair: an insertion taken, a base of the central read deleted)
            assert counters.ins_taken >= 1 and counters.deleted_wins >= 1, counters.as_dict()
        print("locus %d (%d reads): %s" % (k, L["depth"], counters.as_dict()))
