"""Host-side mirror of what `trgt plot` computes per locus before it draws, over the GPU batch ABI trgt_plot_align_batch.

Reference (PacificBiosciences/trgt v3.0.0, src/trvz/):
  get_allele_align   align_allele.rs:7-14        -> get_allele_align(locus, consensus, reads)      (mode 0)
  align (waterfall)  waterfall_plot.rs:28-123    -> waterfall_align(locus, reads)                  (mode 1)
  AlleleAlign / Align / AlignSeg / AlignOp / SegType   align.rs:3-32
Every HMM labelling, alignment, conversion and projection runs in trgt_plot_align_batch (trgt_amd/csrc/plot_align.hip); this module
only packs batches and unpacks results.  Reading the VCF / BAM tags, --max-allele-reads subsampling and rendering stay with the caller.
"""
import ctypes as C

import numpy as np

from . import _lib

MATCH, SUBST, INS, DEL = range(4)          # AlignOp, align.rs:18-24
LEFT_FLANK, RIGHT_FLANK = 0xFFFE, 0xFFFF   # SegType::LeftFlank / RightFlank; SegType::Tr(i) is the integer i
I32_MIN = -2147483648
_VP = C.c_void_p


class PlotIn(C.Structure):  # trgt_plot_in, include/trgt_hip_plot.h
    _fields_ = [("mode", C.c_int32), ("n_sets", C.c_int32), ("motif_blob", _VP), ("motif_off", _VP), ("set_motif_begin", _VP),
                ("n_panels", C.c_int64)] + [(n, _VP) for n in (
                    "panel_set", "ref_blob", "ref_off", "ref_len", "lf_len", "rf_len", "panel_read_begin", "read_blob", "read_off",
                    "read_len", "beta_begin", "beta_pos")]


class PlotOut(C.Structure):  # trgt_plot_out
    _fields_ = [(n, _VP) for n in ("pseg", "pseg_off", "n_pseg", "rseg", "rseg_off", "n_rseg", "beta_proj", "score", "order")]


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def _u8(b):
    return np.frombuffer(b, np.uint8).copy() if len(b) else np.zeros(1, np.uint8)


def seg_capacity(mode, ref_len, read_len):
    """trgt_plot_seg_capacity: segments a slot must hold (no GPU needed)"""
    return int(_lib.lib().trgt_plot_seg_capacity(int(mode), int(ref_len), int(read_len)))


def kernel_ms(ctx=None):
    """trgt_plot_kernel_ms: (plot_motif_segs_kernel, plot_read_segs_kernel) of the context's last timed call, in ms"""
    ctx = ctx or _lib.context()
    out = (C.c_double * 2)()
    ctx.check(_lib.lib().trgt_plot_kernel_ms(ctx.handle, out))
    return float(out[0]), float(out[1])


def pack(mode, panels, with_betas=True):
    """panels: [dict(motifs=, lf=, rf=, ref=, reads=[dict(seq=, betas=[(pos, value)])])] -> the ABI arrays (host).  mode 1: `ref` may be
    left out (it is lf + rf).  One motif set per panel."""
    motifs = [[_b(m) for m in p["motifs"]] for p in panels]
    flat = [m for ms in motifs for m in ms]
    motif_off = np.zeros(len(flat) + 1, np.uint32)
    motif_off[1:] = np.cumsum([len(m) for m in flat])
    set_begin = np.zeros(len(panels) + 1, np.uint32)
    set_begin[1:] = np.cumsum([len(ms) for ms in motifs])
    refs = [_b(p["ref"]) if p.get("ref") is not None else _b(p["lf"]) + _b(p["rf"]) for p in panels]
    ref_len = np.array([len(r) for r in refs], np.uint32)
    ref_off = np.zeros(len(panels), np.uint64)
    ref_off[1:] = np.cumsum(ref_len[:-1], dtype=np.uint64)
    reads = [r for p in panels for r in p["reads"]]
    seqs = [_b(r["seq"]) for r in reads]
    read_len = np.array([len(s) for s in seqs], np.uint32)
    read_off = np.zeros(len(reads), np.uint64)
    if len(reads) > 1:
        read_off[1:] = np.cumsum(read_len[:-1], dtype=np.uint64)
    prb = np.zeros(len(panels) + 1, np.uint64)
    prb[1:] = np.cumsum([len(p["reads"]) for p in panels])
    betas = [list(r.get("betas", [])) for r in reads]
    beta_begin = np.zeros(len(reads) + 1, np.uint64)
    beta_begin[1:] = np.cumsum([len(b) for b in betas])
    beta_pos = np.array([pos for b in betas for pos, _ in b] + [0], np.uint32)
    b = dict(mode=int(mode), n_sets=len(panels), n_panels=len(panels), motif_blob=_u8(b"".join(flat)), motif_off=motif_off, set_motif_begin=set_begin,
             n_motifs=[len(ms) for ms in motifs], panel_set=np.arange(len(panels), dtype=np.uint32), ref_blob=_u8(b"".join(refs)),
             ref_off=ref_off, ref_len=ref_len, lf_len=np.array([len(_b(p["lf"])) for p in panels], np.uint32),
             rf_len=np.array([len(_b(p["rf"])) for p in panels], np.uint32), panel_read_begin=prb, read_blob=_u8(b"".join(seqs)),
             read_off=read_off, read_len=read_len, beta_begin=beta_begin if with_betas else None, beta_pos=beta_pos if with_betas else None,
             beta_values=[[v for _, v in bl] for bl in betas])
    # output layout: one slot of trgt_plot_seg_capacity segments per panel and per read
    read_panel = np.repeat(np.arange(len(panels)), np.diff(prb).astype(np.int64))
    pcap = [seg_capacity(0, int(n), 0) for n in ref_len]
    rcap = [seg_capacity(mode, int(ref_len[read_panel[r]]), int(read_len[r])) for r in range(len(reads))]
    b["pseg_off"] = np.concatenate([[0], np.cumsum(pcap)]).astype(np.uint64)
    b["rseg_off"] = np.concatenate([[0], np.cumsum(rcap)]).astype(np.uint64)
    return b


def alloc_outputs(b, fill=0):
    """host output arrays of a packed batch, pre-filled with `fill` (a byte)"""
    def arr(n, dt):
        a = np.empty(max(int(n), 1), dt)
        a.view(np.uint8)[:] = fill
        return a
    nr, np_ = len(b["read_len"]), b["n_panels"]
    return dict(pseg=arr(2 * int(b["pseg_off"][-1]), np.uint32), n_pseg=arr(np_, np.uint32), rseg=arr(2 * int(b["rseg_off"][-1]), np.uint32),
                n_rseg=arr(nr, np.uint32), beta_proj=arr(len(b["beta_pos"]) if b["beta_pos"] is not None else 1, np.int32), score=arr(nr, np.int32),
                order=arr(nr, np.uint32))


def call(b, outs, ctx=None, ref_blob=None, read_blob=None, check=True):
    """trgt_plot_align_batch on a packed batch.  ref_blob / read_blob: torch uint8 tensors already in HBM, instead of the host blobs;
    outs: host arrays or HBM tensors per output name (None: not wanted).  Returns the call's return code (raises unless check=False)."""
    ctx = ctx or _lib.context()
    p = _lib.ptr
    cin = PlotIn(b["mode"], b["n_sets"], p(b["motif_blob"]), p(b["motif_off"]), p(b["set_motif_begin"]), b["n_panels"], p(b["panel_set"]),
                 p(ref_blob if ref_blob is not None else b["ref_blob"]), p(b["ref_off"]), p(b["ref_len"]), p(b["lf_len"]), p(b["rf_len"]),
                 p(b["panel_read_begin"]), p(read_blob if read_blob is not None else b["read_blob"]), p(b["read_off"]), p(b["read_len"]),
                 p(b["beta_begin"]), p(b["beta_pos"]))
    cout = PlotOut(p(outs.get("pseg")), p(b["pseg_off"]), p(outs.get("n_pseg")), p(outs.get("rseg")), p(b["rseg_off"]), p(outs.get("n_rseg")),
                   p(outs.get("beta_proj")), p(outs.get("score")), p(outs.get("order")))
    rc = _lib.lib().trgt_plot_align_batch(ctx.handle, C.byref(cin), C.byref(cout))
    if check:
        ctx.check(rc)
    return rc


def _segs(words, off, n):
    w = words[2 * off:2 * (off + n)].reshape(-1, 2)
    return [(int(a), int(k) & 0xFF, int(k) >> 8) for a, k in w]


def unpack(b, outs):
    """-> per panel dict(seq=[(width, op, seg_type)] (mode 0), reads=[(align, betas)] in plot order, order=[read index inside the panel],
    scores=[per read, input order]); betas are [(projected position, value)] of the betas project_betas keeps"""
    res = []
    prb = b["panel_read_begin"]
    for p in range(b["n_panels"]):
        r0, r1 = int(prb[p]), int(prb[p + 1])
        aligned = []
        for r in range(r0, r1):
            align = _segs(outs["rseg"], int(b["rseg_off"][r]), int(outs["n_rseg"][r]))
            betas = []
            if b["beta_begin"] is not None:
                b0, b1 = int(b["beta_begin"][r]), int(b["beta_begin"][r + 1])
                betas = [(int(outs["beta_proj"][i]), b["beta_values"][r][i - b0]) for i in range(b0, b1) if outs["beta_proj"][i] >= 0]
            aligned.append((align, betas))
        order = [int(v) - r0 for v in outs["order"][r0:r1]]
        res.append(dict(seq=_segs(outs["pseg"], int(b["pseg_off"][p]), int(outs["n_pseg"][p])) if b["mode"] == 0 else None,
                        reads=[aligned[k] for k in order], order=order, scores=[int(v) for v in outs["score"][r0:r1]]))
    return res


def align_batch(mode, panels, ctx=None):
    """One trgt_plot_align_batch call over `panels` (see pack).  Returns, per panel, dict(seq=, reads=[(align, betas)]) in plot order:
    AlleleAlign for mode 0, the list handed to plot() for mode 1, with the beta values re-attached on the host."""
    if not panels:
        return []
    b = pack(mode, panels)
    outs = alloc_outputs(b)
    call(b, outs, ctx)
    return unpack(b, outs)


def _locus_fields(locus):
    get = (lambda k, alt: locus[k] if k in locus else locus[alt]) if isinstance(locus, dict) else (lambda k, alt: getattr(locus, k))
    return get("left_flank", "lf"), get("right_flank", "rf"), get("motifs", "motifs")


def get_allele_align(locus, consensus, reads, ctx=None):
    """get_allele_align, align_allele.rs:7-14.  locus: left_flank / right_flank / motifs (attributes, or a dict that may also say lf / rf);
    consensus: left flank + allele + right flank; reads: [dict(seq=, betas=[(pos, value)])]"""
    lf, rf, motifs = _locus_fields(locus)
    return align_batch(0, [dict(motifs=motifs, lf=lf, rf=rf, ref=consensus, reads=list(reads))], ctx)[0]


def waterfall_align(locus, reads, ctx=None):
    """The reads of plot_waterfall as it hands them to plot(), waterfall_plot.rs:28-37: sorted by length, each aligned by align (:42-123)"""
    lf, rf, motifs = _locus_fields(locus)
    return align_batch(1, [dict(motifs=motifs, lf=lf, rf=rf, reads=list(reads))], ctx)[0]["reads"]
