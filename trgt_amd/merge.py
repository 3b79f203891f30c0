"""Host-side mirror of what `trgt merge` computes per site between reading N records and writing one, over the batch ABI
trgt_merge_exact_batch / trgt_merge_exact_host (include/trgt_hip_merge.h).

Reference (PacificBiosciences/trgt v3.0.0):
  merge_exact   src/merge/strategy/exact.rs:6-88   -> merge_exact(vcf_gts, sample_alleles)   one site, the reference's signature
                                                      exact_batch(sites)                      many sites in one call
The de-duplication, the (length, bytes) order and the rewriting of the GT indices run in trgt_merge_exact_batch
(trgt_amd/csrc/merge_exact.hip) when a context is given and in its host twin trgt_merge_exact_host otherwise; this module only packs
batches and unpacks results.  Reading the VCFs, the heap over positions, the padding of pre-1.0 files, header merging, the FORMAT
concatenation of process_format_fields and writing stay with the caller.

Genotype values.  exact_batch takes and returns them in BCF encoding (ints): (i + 1) << 1 Unphased(i), ((i + 1) << 1) | 1 Phased(i), 0
UnphasedMissing, 1 PhasedMissing, VECTOR_END passed through.  merge_exact takes GenotypeAllele as tuples: ("U", i) Unphased(i), ("P", i)
Phased(i), ("U", None) UnphasedMissing, ("P", None) PhasedMissing.
"""
import ctypes as C

import numpy as np

from . import _lib

VECTOR_END = -2147483647   # TRGT_MERGE_GT_VECTOR_END, bcf_int32_vector_end
REF_MISMATCH, NO_REF, GT_OUT_OF_RANGE = 1, 2, 3   # site_status
_VP = C.c_void_p
_NEGATIVE = (1 << 29)      # merge_exact: the index a negative GenotypeAllele index is sent as (beyond every entry, so the site gets status 3)


class MergeIn(C.Structure):  # trgt_merge_in, include/trgt_hip_merge.h
    _fields_ = [("n_sites", C.c_int64), ("site_entry_begin", _VP), ("entry_allele_begin", _VP), ("allele_off", _VP), ("allele_len", _VP),
                ("allele_blob", _VP), ("blob_len", C.c_uint64), ("entry_gt_begin", _VP), ("gt", _VP)]


class MergeOut(C.Structure):  # trgt_merge_out
    _fields_ = [(n, _VP) for n in ("site_status", "out_n_alleles", "out_allele_src", "out_allele_begin", "allele_map", "gt_out")]


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def site_alleles_limit():
    """trgt_merge_site_alleles_limit: the largest site (input alleles) the device takes; larger ones go to the host twin (no GPU needed)"""
    return int(_lib.lib().trgt_merge_site_alleles_limit())


def kernel_ms(ctx=None):
    """trgt_merge_kernel_ms: (merge_hash_kernel, merge_site_kernel) of the context's last timed call, in ms"""
    ctx = ctx or _lib.context()
    out = (C.c_double * 2)()
    ctx.check(_lib.lib().trgt_merge_kernel_ms(ctx.handle, out))
    return float(out[0]), float(out[1])


def gt_encode(g):
    """("U" | "P", index or None) -> the BCF value"""
    kind, i = g
    phased = 1 if kind == "P" else 0
    if i is None:
        return phased
    return ((min(int(i), _NEGATIVE) if i >= 0 else _NEGATIVE) + 1) << 1 | phased


def gt_decode(v):
    v = int(v)
    return ("P" if v & 1 else "U", None if v < 2 else (v >> 1) - 1)


def pack(sites, pad=(0,)):
    """sites: [(entries_alleles, entries_gts)] -- per entry the list of its alleles (bytes or str, REF first; [] for a file without a record
    there) and the flat list of its genotype values (ints) -> the ABI arrays (host).  The alleles lie in the blob in input order; allele k
    is preceded by pad[k % len(pad)] filler bytes (tests move sequences across dword boundaries with it).  Every site gets the slot it
    needs: 1 + its ALT alleles, at least 2."""
    seb, eab, egb, slot = [0], [0], [0], [0]
    seqs, gts = [], []
    for alleles, egts in sites:
        assert len(alleles) == len(egts), "one list of genotype values per entry"
        n_alt = 0
        for al, g in zip(alleles, egts):
            seqs.extend(_b(a) for a in al)
            gts.extend(int(v) for v in g)
            eab.append(len(seqs))
            egb.append(len(gts))
            n_alt += max(len(al) - 1, 0)
        seb.append(len(eab) - 1)
        slot.append(slot[-1] + max(1 + n_alt, 2))
    off, pieces, at = [], [], 0
    for k, s in enumerate(seqs):
        p = int(pad[k % len(pad)])
        pieces.append(b"N" * p)
        at += p
        off.append(at)
        pieces.append(s)
        at += len(s)
    blob = b"".join(pieces)
    u64 = lambda v: np.array(v, np.uint64)  # noqa: E731
    return dict(n_sites=len(sites), site_entry_begin=u64(seb), entry_allele_begin=u64(eab), entry_gt_begin=u64(egb), out_allele_begin=u64(slot),
                allele_off=u64(off + [0])[:max(len(off), 1)], allele_len=np.array([len(s) for s in seqs] + [0], np.uint32)[:max(len(seqs), 1)],
                allele_blob=np.frombuffer(blob, np.uint8).copy() if blob else np.zeros(1, np.uint8), blob_len=len(blob),
                gt=np.array(gts + [0], np.int32)[:max(len(gts), 1)], n_alleles=len(seqs), n_gt=len(gts), seqs=seqs)


OUT_NAMES = ("site_status", "out_n_alleles", "out_allele_src", "allele_map", "gt_out")


def alloc_outputs(b, fill=0):
    """host output arrays of a packed batch, pre-filled with `fill` (a byte)"""
    def arr(n):
        a = np.empty(max(int(n), 1), np.int32)
        a.view(np.uint8)[:] = fill
        return a
    return dict(site_status=arr(b["n_sites"]), out_n_alleles=arr(b["n_sites"]), out_allele_src=arr(b["out_allele_begin"][-1]),
                allele_map=arr(b["n_alleles"]), gt_out=arr(b["n_gt"]))


def call(b, outs, ctx=None, blob=None, check=True):
    """trgt_merge_exact_batch (ctx given) or trgt_merge_exact_host (ctx None) on a packed batch.  blob: a torch uint8 tensor already in
    HBM, instead of the host blob; outs: host arrays or HBM tensors per output name.  Returns the return code (raises unless check=False)."""
    p = _lib.ptr
    cin = MergeIn(b["n_sites"], p(b["site_entry_begin"]), p(b["entry_allele_begin"]), p(b["allele_off"]), p(b["allele_len"]),
                  p(blob if blob is not None else b["allele_blob"]), b["blob_len"], p(b["entry_gt_begin"]), p(b["gt"]))
    cout = MergeOut(p(outs.get("site_status")), p(outs.get("out_n_alleles")), p(outs.get("out_allele_src")), p(b["out_allele_begin"]),
                    p(outs.get("allele_map")), p(outs.get("gt_out")))
    L = _lib.lib()
    if ctx is None:
        rc = L.trgt_merge_exact_host(C.byref(cin), C.byref(cout))
        if rc != 0 and check:
            raise _lib.TrgtHipError("libtrgt_hip error %d: %s" % (rc, L.trgt_hip_last_error(None).decode()))
        return rc
    rc = L.trgt_merge_exact_batch(ctx.handle, C.byref(cin), C.byref(cout))
    if check:
        ctx.check(rc)
    return rc


def unpack(b, outs):
    """-> per site (status, alleles, gts): the merged alleles as bytes in output order (status 1: the two REFs that differ; 2, 3: []) and per
    entry the rewritten genotype values (None for a site with a status)"""
    res = []
    seb, eab, egb, slot = b["site_entry_begin"], b["entry_allele_begin"], b["entry_gt_begin"], b["out_allele_begin"]
    for s in range(b["n_sites"]):
        status = int(outs["site_status"][s])
        n = 2 if status == REF_MISMATCH else int(outs["out_n_alleles"][s])
        alleles = [b["seqs"][int(a)] for a in outs["out_allele_src"][int(slot[s]):int(slot[s]) + n]]
        gts = None
        if status == 0:
            gts = [[int(v) for v in outs["gt_out"][int(egb[e]):int(egb[e + 1])]] for e in range(int(seb[s]), int(seb[s + 1]))]
        res.append((status, alleles, gts))
    return res


def exact_batch(sites, ctx=None):
    """merge_exact for every site of `sites` (see pack) in one call: on the device of `ctx`, or by the host twin when ctx is None.
    Returns per site (status, alleles, gts) (see unpack); a site's status never fails the call."""
    if not sites:
        return []
    b = pack(sites)
    outs = alloc_outputs(b)
    call(b, outs, ctx)
    return unpack(b, outs)


def merge_exact(vcf_gts, sample_alleles, ctx=None):
    """merge_exact, exact.rs:6-88, for one site.  vcf_gts[i][sample] is the list of GenotypeAllele tuples of one sample of input i,
    sample_alleles[i] the alleles of input i (REF first, [] when the file has no record).  Returns (out_gts, sorted_alleles); raises
    ValueError with the reference's message where the reference returns Err."""
    flat = [[gt_encode(g) for sample in entry for g in sample] for entry in vcf_gts]
    status, alleles, gts = exact_batch([(list(sample_alleles), flat)], ctx)[0]
    if status == REF_MISMATCH:
        raise ValueError("Reference alleles do not match: '%s' and '%s'" % tuple(a.decode("utf-8", "replace") for a in alleles))
    if status == NO_REF:
        raise ValueError("No reference allele found")
    if status == GT_OUT_OF_RANGE:
        for entry, al in zip(vcf_gts, sample_alleles):
            for sample in entry:
                for _, i in sample:
                    if i is not None and i < 0:
                        raise ValueError("Index out of range: %d" % i)
                    if i is not None and i >= len(al):
                        raise ValueError("Index out of bounds or allele not found in index: None")
    out, k = [], 0
    for entry, vals in zip(vcf_gts, gts):
        k = 0
        samples = []
        for sample in entry:
            samples.append([gt_decode(v) for v in vals[k:k + len(sample)]])
            k += len(sample)
        out.append(samples)
    return out, alleles
