"""What a vote group takes from the three arenas of a consensus repair -- gt::group_needs of trgt_amd/csrc/repair_queue.hpp, the one place
every device genotyper computes it -- restated in Python and checked against values worked out by hand at the edges of its formulas.  No GPU.
The function itself is device code with no host entry point, so this file pins the restatement, not the header: what ties the two together
are the GPU tests of tests/test_repair_queue_gpu.py, whose caps come from this restatement, and the lists repair_check_kernel walks.
tests/test_repair_queue_gpu.py uses the restatement to work out, from the segment lengths of its cases, caps that leave no room."""

U32, U64 = (1 << 32) - 1, (1 << 64) - 1
VOTE_LDS_POS = 4000  # vote::VOTE_LDS_POS (consensus_vote.hpp)


def group_needs(bb, nm, mbytes, vote_lds_pos=VOTE_LDS_POS):
    """(cig words, out_cap bytes, out_need bytes, scr_need words) of a group of nm members, mbytes bytes in all, around a backbone of bb
    bytes: 64-bit sums, out_cap a 32-bit field of the group's record"""
    cig = (nm * (bb + 1) + mbytes) & U64
    out_cap = (bb + mbytes + 16) & U32
    out_need = (out_cap + 15) & ~15
    scr_need = (0 if ((bb + 1) & U32) <= ((vote_lds_pos + 1) & U32) else 3 * (bb + 1)) + 3 * nm
    return cig, out_cap, out_need, scr_need


def test_one_member():
    # one CIGAR slot of bb + len + 1 words; the result: backbone + member + 16, in a 16-aligned slot; three scratch words per member
    assert group_needs(5, 1, 7) == (5 + 7 + 1, 28, 32, 3)


def test_vote_scratch_only_beyond_the_lds_positions():
    # bb + 1 == vote_lds_pos + 1: the votes of every backbone position (and the one behind the last) fit the LDS of the vote kernel
    assert group_needs(4000, 2, 8000)[3] == 3 * 2
    assert group_needs(4001, 2, 8000)[3] == 3 * 4002 + 3 * 2
    assert group_needs(10, 4, 40, vote_lds_pos=10)[3] == 12 and group_needs(11, 4, 40, vote_lds_pos=10)[3] == 3 * 12 + 12


def test_result_slot_is_16_aligned():
    assert group_needs(10, 2, 22)[1:3] == (48, 48)  # a multiple of 16 stays
    assert group_needs(10, 2, 23)[1:3] == (49, 64)  # one above takes the next slot


def test_members_of_4_gib_sum_in_64_bits():
    # the CIGAR words are a 64-bit sum; out_cap is the 32-bit field of RGroup (the envelope -- max_seg, the reads of a locus -- keeps real
    # groups far below it)
    cig, out_cap, out_need, scr = group_needs(100, 3, (1 << 32) - 50)
    assert cig == 3 * 101 + (1 << 32) - 50 and cig > U32
    assert (out_cap, out_need) == (66, 80) and scr == 9


def test_needs_of_a_locus_add_up():
    # two groups of one locus are reserved as one block per arena: the sums of the groups' needs
    a, b = group_needs(60, 5, 300), group_needs(63, 3, 190)
    assert a == (5 * 61 + 300, 376, 384, 15) and b == (3 * 64 + 190, 269, 272, 9)
