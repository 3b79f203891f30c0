"""The haplotype-tag route of the deep size genotyper adds no entry point: the two existing settings combine, out[3] of
trgt_hip_flank_stats gets its meaning, ABI 11 stays.  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _comment_before(text, decl):
    return text[:text.index(decl)].rsplit("/*", 1)[1]


def test_header_describes_out3_and_the_new_envelope():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    flank = _comment_before(text, "int trgt_hip_set_flank_device")
    assert re.search(r"out\[3\]", flank) and "reserved" not in flank.split("out[3]")[1][:200]
    assert "trgt_hip_set_size_max_reads" in flank
    # "more than 256 reads" is no longer listed as the host's without the qualification
    for m in re.finditer(r"more than 256 (candidate )?reads", flank):
        around = flank[max(0, m.start() - 300):m.end() + 300]
        assert "trgt_hip_set_size_max_reads" in around or "size_max_reads" in around, around
    size = _comment_before(text, "int trgt_hip_set_size_max_reads")
    assert "trgt_hip_set_flank_device" in size


def test_chunk_driver_sets_both_on_every_context():
    from trgt_amd import driver

    class Ctx:
        def __init__(self):
            self.flank = self.size = None

        def set_flank_device(self, on):
            self.flank = on

        def set_size_max_reads(self, n):
            self.size = n

    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_device=True, size_max_reads=750)
    assert [(c.flank, c.size) for c in d.contexts] == [(True, 750), (True, 750)]


def test_abi_is_still_11_and_no_new_export():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_abi_version() == 11
    assert sorted(n for n in _lib.EXPORTS if n.startswith("trgt_hip_") and "flank" in n) == ["trgt_hip_flank_stats", "trgt_hip_set_flank_device"]
