"""The plot path's three entry points (include/trgt_hip_plot.h): names, declarations, the loader's list, and trgt_plot_seg_capacity held
against the segment counts of every designed case.  No GPU."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["trgt_plot_align_batch", "trgt_plot_seg_capacity", "trgt_plot_kernel_ms"]


def uncommented(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_plot_exports_are_exactly_the_three_functions():
    from trgt_amd import _lib
    assert sorted(_lib.PLOT_EXPORTS) == sorted(NAMES)
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), "libtrgt_hip.so does not export %s" % n
    # a list of its own: EXPORTS stays the names include/trgt_hip.h itself declares, and the ABI version stays
    assert not set(NAMES) & set(_lib.EXPORTS)
    main_h = uncommented(os.path.join(ROOT, "include", "trgt_hip.h"))
    assert sorted(_lib.EXPORTS) == sorted(set(re.findall(r"\b(trgt_[a-z0-9_]+)\s*\(", main_h)))
    assert L.trgt_hip_abi_version() == 11


def test_header_declares_them_and_trgt_hip_h_includes_it():
    plot_h = uncommented(os.path.join(ROOT, "include", "trgt_hip_plot.h"))
    assert sorted(set(re.findall(r"\b(trgt_[a-z0-9_]+)\s*\(", plot_h))) == sorted(NAMES)
    for field in ("mode", "n_sets", "motif_blob", "motif_off", "set_motif_begin", "n_panels", "panel_set", "ref_blob", "ref_off", "ref_len", "lf_len", "rf_len",
                  "panel_read_begin", "read_blob", "read_off", "read_len", "beta_begin", "beta_pos", "pseg", "pseg_off", "n_pseg", "rseg", "rseg_off", "n_rseg",
                  "beta_proj", "score", "order"):
        assert re.search(r"\b%s\b" % field, plot_h), field
    main_h = uncommented(os.path.join(ROOT, "include", "trgt_hip.h"))
    assert '#include "trgt_hip_plot.h"' in main_h
    assert not any(n in main_h for n in NAMES)   # (outside comments trgt_hip.h names none of them: tests/test_abi_exports.py compares its names with EXPORTS)


def test_python_structs_mirror_the_header():
    from trgt_amd import plot
    plot_h = uncommented(os.path.join(ROOT, "include", "trgt_hip_plot.h"))
    for cls, name in ((plot.PlotIn, "trgt_plot_in"), (plot.PlotOut, "trgt_plot_out")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), plot_h, flags=re.S).group(1)
        fields = re.findall(r"\b(\w+)\s*[;,]", body)
        assert [f for f, _ in cls._fields_] == fields, (name, fields)


def test_seg_capacity_formulas_and_designed_cases():
    import plot_cases as pc
    from trgt_amd import plot
    assert plot.seg_capacity(0, 100, 50) == 2 * 100 + 50 + 3
    assert plot.seg_capacity(0, 100, 0) == 203
    assert plot.seg_capacity(1, 100, 160) == 2 * 160 + 2
    assert plot.seg_capacity(0, 0xFFFFFFFF, 0xFFFFFFFF) == 3 * 0xFFFFFFFF + 3   # no 32-bit wrap
    for case in pc.cases():
        p, exp = case["panel"], pc.expected(case)
        if case["mode"] == 0:
            assert len(exp["seq"]) <= plot.seg_capacity(0, len(p["ref"]), 0), case["name"]
        for k, (align, _) in zip(exp["order"], exp["reads"]):
            assert len(align) <= plot.seg_capacity(case["mode"], len(p["ref"]), len(p["reads"][k]["seq"])), (case["name"], k)
