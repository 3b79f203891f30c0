"""The SNV branch of genotype_flank for deep size loci adds no entry point, no environment switch and no Python argument: it is reached by
combining trgt_hip_set_snv_split_device with trgt_hip_set_size_max_reads.  ABI 11 stands, the exports are the functions trgt_hip.h
declares, the header says what out[3] of trgt_hip_size_deep_stats means, and ChunkDriver hands both settings to every context.  No GPU
needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    return text + open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()


def _comment_before(text, decl):
    return " ".join(text[:text.index(decl)].rsplit("/*", 1)[1].replace("\n *", " ").split())


def test_abi_is_still_11_and_the_exports_are_the_declared_functions():
    from trgt_amd import _lib
    assert _lib.lib().trgt_hip_abi_version() == 11
    declared = set(re.findall(r"\b(trgt_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)))
    exports = list(_lib.EXPORTS) + list(_lib.CLUSTER_FLANK_EXPORTS)
    assert len(exports) == len(set(exports))
    assert set(exports) <= declared, sorted(set(exports) - declared)
    assert not any("snv_deep" in n or "deep_snv" in n for n in declared)  # no entry point of its own
    assert sorted(n for n in _lib.EXPORTS if "snv" in n) == ["trgt_hip_set_snv_split_device", "trgt_hip_snv_split_stats"]
    assert sorted(n for n in _lib.EXPORTS if "size_" in n) == ["trgt_hip_set_size_max_reads", "trgt_hip_size_deep_stats", "trgt_hip_size_max_reads_limit"]
    assert not any("SNV" in k for k in _lib.RELEASE_KNOBS)  # no environment switch either


def test_header_says_what_out3_means_and_that_the_settings_combine():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    size = _comment_before(text, "int32_t trgt_hip_size_max_reads_limit")
    assert "out[3] those of out[0] that the SNV branch settled on the device" in size and "out[3] reserved" not in size
    assert "trgt_hip_set_snv_split_device" in size and "combine" in size
    snv = _comment_before(text, "int trgt_hip_set_snv_split_device")
    assert "combines with trgt_hip_set_size_max_reads" in snv and "locus_gt_deep.hpp" in snv and "16384" in snv
    for stays in ("Genotyper::Cluster", "beyond that setting or the 2048-read ceiling", "not decided beyond the margin", "64 called SNVs",
                  "16 distinct fully observed profiles", "8 in-region mismatch offsets", "TRGT_REPAIR_MAX_SEG", "TRGT_HOST_REPAIR", "allele_cap"):
        assert stays in snv, stays
    flank = _comment_before(text, "int trgt_hip_set_flank_device")
    assert "trgt_hip_set_snv_split_device" in flank and "tags first" in flank


def test_python_docstrings_follow():
    from trgt_amd import _lib, driver
    assert "set_size_max_reads" in _lib.Context.set_snv_split_device.__doc__
    assert "SNV" in _lib.Context.size_deep_stats.__doc__ and "Deep size loci" in _lib.Context.snv_split_stats.__doc__
    assert "snv_split_device combine" in driver.ChunkDriver.__doc__


def test_chunk_driver_passes_both_settings_to_every_context():
    from trgt_amd import driver

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_snv_split_device(self, on):
            self.calls.append(("snv", on))

        def set_size_max_reads(self, n):
            self.calls.append(("size", n))

    d = driver.ChunkDriver(devices=(0, 0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, snv_split_device=True, size_max_reads=750)
    assert [sorted(c.calls) for c in d.contexts] == [[("size", 750), ("snv", True)]] * 3
