"""The five device routes of genotype_flank share one table on either side of the C ABI (FlankRoute in trgt_amd/csrc/common.hpp, ROUTES
in trgt_amd/_lib.py).  Without a GPU: the ten entry points refuse null arguments alike, and the Python table generates the ten Context
methods with the documented names, defaults and docstrings."""
import ctypes as C
import inspect

import pytest

from trgt_amd import _lib

TRGT_ERR_INVALID = -1
NAMES = ("flank", "snv_split", "flank_cluster", "flank_cluster_deep", "snv_cluster")


def test_the_table_names_the_ten_entry_points_once():
    assert tuple(r[0] for r in _lib.ROUTES) == NAMES
    exported = _lib.EXPORTS + _lib.CLUSTER_FLANK_EXPORTS + _lib.CLUSTER_SNV_EXPORTS + _lib.CLUSTER_DEEP_FLANK_EXPORTS
    for name, setter, stats, width, _, _ in _lib.ROUTES:
        assert (setter, stats) == ("trgt_hip_set_%s_device" % name, "trgt_hip_%s_stats" % name)
        assert exported.count(setter) == 1 and exported.count(stats) == 1
        assert width == (3 if name.startswith("flank_cluster") else 4)


@pytest.mark.parametrize("row", _lib.ROUTES, ids=NAMES)
def test_entry_points_refuse_null_arguments(row):
    _, setter, stats, width, _, _ = row
    L = _lib.lib()
    assert getattr(L, setter)(None, 1) == TRGT_ERR_INVALID
    out = (C.c_int64 * width)(*[7] * width)
    assert getattr(L, stats)(None, out) == TRGT_ERR_INVALID and list(out) == [7] * width
    assert getattr(L, stats)(None, None) == TRGT_ERR_INVALID


@pytest.mark.parametrize("row", _lib.ROUTES, ids=NAMES)
def test_context_methods_come_from_the_table(row):
    name, setter, stats, width, set_doc, stats_doc = row
    set_m, stats_m = getattr(_lib.Context, "set_%s_device" % name), getattr(_lib.Context, "%s_stats" % name)
    assert (set_m.__name__, stats_m.__name__) == ("set_%s_device" % name, "%s_stats" % name)
    assert list(inspect.signature(set_m).parameters) == ["self", "on"] and inspect.signature(set_m).parameters["on"].default is True
    assert list(inspect.signature(stats_m).parameters) == ["self"]
    assert set_m.__doc__ == set_doc and set_doc.startswith(setter + ":")
    assert stats_m.__doc__ == stats_doc and stats_doc.startswith(stats + " of the context's last trgt_locus_batch")


def test_apply_settings_skips_what_was_not_given_and_keeps_the_order():
    class Ctx:
        def __init__(self):
            self.calls = []

        def a(self, v):
            self.calls.append(("a", v))

        def b(self, v):
            self.calls.append(("b", v))

    ctxs = [Ctx(), Ctx()]
    _lib.apply_settings(ctxs, ((False, "b"), (None, "missing"), (3, "a")))
    assert all(c.calls == [("b", False), ("a", 3)] for c in ctxs)
