"""The deep instantiation of the device-side size genotyper is an addition to ABI 11: three new entry points, no GPU needed to ask for
the compiled ceiling."""
import ctypes as C


def test_size_max_reads_symbols_and_ceiling():
    from trgt_amd import _lib
    L = _lib.lib()
    for name in ("trgt_hip_size_max_reads_limit", "trgt_hip_set_size_max_reads", "trgt_hip_size_deep_stats"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
    assert L.trgt_hip_size_max_reads_limit() >= 2048
    assert _lib.size_max_reads_limit() == L.trgt_hip_size_max_reads_limit()
    assert L.trgt_hip_abi_version() == 11


def test_setter_and_stats_refuse_a_null_context():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_size_max_reads(None, 512) != 0
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.trgt_hip_size_deep_stats(None, out) != 0
    assert list(out) == [7, 7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    assert "size_max_reads" in inspect.signature(_lib.Pool.__init__).parameters
    assert "size_max_reads" in inspect.signature(driver.ChunkDriver.__init__).parameters
    assert callable(_lib.Context.set_size_max_reads) and callable(_lib.Context.size_deep_stats)
