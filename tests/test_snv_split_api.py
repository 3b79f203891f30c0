"""The SNV branch of genotype_flank on the device is an addition to ABI 11: two new entry points, declared in trgt_hip.h itself, listed
in the loader's exports and wrapped by the Python layers.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trgt_hip_set_snv_split_device", "trgt_hip_snv_split_stats")


def test_header_declares_both_functions_and_says_what_stays_on_the_host():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    assert re.search(r"int\s+trgt_hip_set_snv_split_device\(trgt_hip_ctx\*\s*ctx,\s*int\s+on\);", text)
    assert re.search(r"int\s+trgt_hip_snv_split_stats\(const trgt_hip_ctx\*\s*ctx,\s*int64_t\s+out\[4\]\);", text)
    assert text.index('#include "trgt_hip_flank_cluster.h"') < text.index("int trgt_hip_set_snv_split_device")
    comment = " ".join(text[:text.index("int trgt_hip_set_snv_split_device")].rsplit("/*", 1)[1].replace("\n *", " ").split())
    assert "genotype_flank.rs:78-138, 171-290" in comment and "tr.rs:69-75" in comment
    for stays in ("Genotyper::Cluster", "more than 256 reads", "TRGT_HOST_GENOTYPER", "trgt_hip_set_flank_device is off", "not decided beyond the margin",
                  "TRGT_REPAIR_MAX_SEG", "TRGT_HOST_REPAIR", "allele_cap", "64 called SNVs", "16 distinct fully observed profiles", "8 in-region mismatch offsets"):
        assert stays in comment, stays
    assert all("flank" not in n for n in NAMES)


def test_a_c_program_that_includes_the_header_has_the_prototypes(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "trgt_hip.h"\n'
                   "int use(trgt_hip_ctx* c) { int64_t out[4]; int (*set)(trgt_hip_ctx*, int) = trgt_hip_set_snv_split_device;\n"
                   "  int (*get)(const trgt_hip_ctx*, int64_t*) = trgt_hip_snv_split_stats; return set(c, 1) + get(c, out); }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_library_exports_them_at_abi_11():
    from trgt_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and name not in _lib.CLUSTER_FLANK_EXPORTS and hasattr(L, name), name
    assert L.trgt_hip_abi_version() == 11


def test_setter_and_stats_refuse_a_null_context():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_snv_split_device(None, 1) != 0
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.trgt_hip_snv_split_stats(None, out) != 0
    assert list(out) == [7, 7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    for f in (_lib.Pool.__init__, driver.ChunkDriver.__init__):
        p = inspect.signature(f).parameters
        assert "snv_split_device" in p and p["snv_split_device"].default is None
    assert inspect.signature(_lib.Context.set_snv_split_device).parameters["on"].default is True
    assert callable(_lib.Context.snv_split_stats)


def test_chunk_driver_passes_the_setting_and_leaves_the_other_two_alone():
    from trgt_amd import driver

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_snv_split_device(self, on):
            self.calls.append(("snv", on))

        def set_flank_device(self, on):
            self.calls.append(("flank", on))

        def set_flank_cluster_device(self, on):
            self.calls.append(("flank cluster", on))

    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, snv_split_device=True)
    assert [c.calls for c in d.contexts] == [[("snv", True)]] * 2
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_device=True)
    assert [c.calls for c in d.contexts] == [[("flank", True)]]

    class Bare:  # a context fake without the setter: never called when the argument is None
        pass

    driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Bare(), run_fn=lambda *a: None)
