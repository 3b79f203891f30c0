"""The haplotype-tag branch of genotype_flank on the device is an addition to ABI 11: two new entry points, declared in the header,
listed in the loader's exports and wrapped by the Python layers.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trgt_hip_set_flank_device", "trgt_hip_flank_stats")


def test_header_declares_both_functions_and_says_what_stays_on_the_host():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    assert re.search(r"int\s+trgt_hip_set_flank_device\(trgt_hip_ctx\*\s*ctx,\s*int\s+on\);", text)
    assert re.search(r"int\s+trgt_hip_flank_stats\(const trgt_hip_ctx\*\s*ctx,\s*int64_t\s+out\[4\]\);", text)
    comment = text[:text.index("int trgt_hip_set_flank_device")].rsplit("/*", 1)[1]
    assert "genotype_flank.rs:43-76" in comment and "tr.rs:69-75" in comment and "get_trs_with_clustering" in comment


def test_library_exports_them_at_abi_11():
    from trgt_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.trgt_hip_abi_version() == 11


def test_setter_and_stats_refuse_a_null_context():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_flank_device(None, 1) != 0
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.trgt_hip_flank_stats(None, out) != 0
    assert list(out) == [7, 7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    assert "flank_device" in inspect.signature(_lib.Pool.__init__).parameters
    assert "flank_device" in inspect.signature(driver.ChunkDriver.__init__).parameters
    assert callable(_lib.Context.set_flank_device) and callable(_lib.Context.flank_stats)


def test_chunk_driver_passes_the_setting_to_every_context():
    from trgt_amd import driver

    class Ctx:
        def __init__(self):
            self.flank = None

        def set_flank_device(self, on):
            self.flank = on

    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_device=True)
    assert [c.flank for c in d.contexts] == [True, True]
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None)
    assert [c.flank for c in d.contexts] == [None]
