"""trgt_writer_set_records_device / trgt_writer_records_stats (additive to ABI 11) where no GPU is needed: the exports, and the rule that a
device that cannot be used fails the call instead of leaving a host-only writer behind (the GPU side: test_writer_records_device_gpu.py)."""
import ctypes as C

import pytest

from test_ingest import _synthetic


def test_exports():
    from trgt_amd import _lib
    L = _lib.lib()
    for n in ("trgt_writer_set_records_device", "trgt_writer_records_stats"):
        assert n in _lib.EXPORTS and hasattr(L, n), n
    assert L.trgt_hip_abi_version() == 11


def test_an_unusable_records_device_fails_the_setter(tmp_path):
    import torch
    from trgt_amd import _lib, ingest, writers
    bam, fa, bed, recs, genome = _synthetic(tmp_path)
    rd = ingest.Reader(bam, fa)
    # no GPU here: ordinal 0 cannot be used; with one: ordinal 99 cannot
    dev = 99 if torch.cuda.is_available() else 0
    with pytest.raises(_lib.TrgtHipError, match="records_device %d" % dev):
        writers.Writer(rd, tmp_path / "a.vcf", tmp_path / "a.bam", records_device=dev)
    # through the C ABI on an open writer: an error code and a message, and the writer goes on as it was (host formatting, counted as nothing)
    w = writers.Writer(rd, tmp_path / "b.vcf", tmp_path / "b.bam")
    L = _lib.lib()
    L.trgt_writer_set_records_device.argtypes = [C.c_void_p, C.c_int32]
    assert L.trgt_writer_set_records_device(w.handle, dev) < 0
    assert ("records_device %d" % dev) in L.trgt_writer_last_error(w.handle).decode()
    assert L.trgt_writer_set_records_device(w.handle, -1) == 0   # off: what open leaves
    assert w.records_stats() == dict(device_batches=0, host_batches=0, host_reason=0, records=0, bytes=0)
    w.close()
    # a writer without a spanning BAM has no records to assemble
    with pytest.raises(_lib.TrgtHipError, match="without a spanning BAM"):
        writers.Writer(rd, tmp_path / "c.vcf", None, records_device=0)
