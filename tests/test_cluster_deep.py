"""The deep instantiation of the device-side cluster genotyper is an addition to ABI 11: two new entry points, no GPU needed to ask for
the compiled ceiling."""


def test_cluster_max_reads_symbols_and_ceiling():
    from trgt_amd import _lib
    L = _lib.lib()
    for name in ("trgt_hip_cluster_max_reads_limit", "trgt_hip_set_cluster_max_reads"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
    assert L.trgt_hip_cluster_max_reads_limit() >= 2048
    assert _lib.cluster_max_reads_limit() == L.trgt_hip_cluster_max_reads_limit()
    assert L.trgt_hip_abi_version() == 11


def test_setter_refuses_a_null_context():
    from trgt_amd import _lib
    assert _lib.lib().trgt_hip_set_cluster_max_reads(None, 512) != 0
